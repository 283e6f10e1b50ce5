"""GPU: vdr_op_knn (csrc/knn.hip) at op level against the float64 statement of tests/knn_ref.py, and what is built on it
(vdr.knn.search / KnnClassifier, VitDescriptorModel.transfer_labels / fit_knn / knn_predict, MemoryBank.score(k)).

Designed inputs (nn_cosine_ref.designed: 16 entries of +-1 per row, every cosine a multiple of 1/16, every squared distance the
integer 32 - 2 dot) must come back bit for bit, ties in index order, for both metrics, with and without the excluded diagonal:
tq 1 / 127 / 129 / 300 (one lane, the ragged panel on both sides of 128, three panels), tc k / 64 / 129 / 700 (every candidate
returned; one row wave empty; the ragged second tile; 6 tiles, so the run split and the merge of the partial lists), d 32 / 96 /
448 (half a K step, the short last step, an odd number of steps), k 1 / 4 / 5 / 8 / 9 / 16 (both sides of every list length),
pairs 1 and 3.  tc == k with exclude_diag leaves k - 1 eligible candidates: the refusal is what is asserted there.
Random inputs (knn_ref.planted) go through knn_ref.check_near_tie_tolerant, with floors on the share of clear rows of the
REFERENCE; the golden files hold scikit-learn's answers on clear rows."""
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
import knn_ref as kr
import memguard as mg
import nn_cosine_ref as nref
from fixtures import ops  # noqa: F401
from handle_configs import TINY
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

KS = (1, 4, 5, 8, 9, 16)
PAIRS = 3
_CACHE = {}


def _designed(tq, tc, d):
    """(q, c bf16 on the device, {(metric, diag): (float64 scores, stable order of the first 16)}) of 3 problems: once per shape"""
    key = (tq, tc, d)
    if key not in _CACHE:
        q, c = nref.designed(PAIRS, tq, tc, d, seed=20000 * tq + 20 * tc + d)
        ref = {}
        for metric in kr.METRICS:
            s = kr.scores(q, c, metric)
            for diag in (False, True):
                ref[metric, diag] = (s, np.argsort(kr.cost(s, metric, diag), axis=-1, kind="stable")[..., :16])
        _CACHE[key] = (q.to(torch.bfloat16).cuda(), c.to(torch.bfloat16).cuda(), ref)
    return _CACHE[key]


def _exact(got, s, order, k, P, what):
    val, idx = (t.cpu().numpy() for t in got)
    assert val.dtype == np.float32 and idx.dtype == np.int32 and val.shape == idx.shape == (P,) + s.shape[1:2] + (k,), what
    want_idx = order[:P, :, :k]
    assert np.array_equal(idx, want_idx), (what, "idx", np.argwhere(idx != want_idx)[:4].tolist())
    assert np.array_equal(val.astype(np.float64), np.take_along_axis(s[:P], want_idx, -1)), (what, "val")
    assert not np.signbit(val[val == 0]).any() or what[0] == "cosine", (what, "-0 returned")


@pytest.mark.parametrize("d", (32, 96, 448))
@pytest.mark.parametrize("tq", (1, 127, 129, 300))
def test_designed_inputs_are_exact(ops, tq, d):
    ties = 0
    for k in KS:
        for tc in (k, 64, 129, 700):
            q, c, ref = _designed(tq, tc, d)
            for metric in kr.METRICS:
                for diag in (False, True):
                    s, order = ref[metric, diag]
                    if tc - int(diag) < k:
                        with pytest.raises(ValueError, match="fewer than k"):
                            ops.knn(q, c, k, metric, diag)
                        continue
                    if tc >= 64 and k > 1:
                        top = np.take_along_axis(s, order[..., :k], -1)
                        ties += int((top[..., 1:] == top[..., :-1]).sum())
                    for P in (1, PAIRS):
                        _exact(ops.knn(q[:P], c[:P], k, metric, diag), s, order, k, P, (metric, diag, tq, tc, d, k, P))
    assert ties > 0  # (something to see: equal scores inside the returned lists)


def test_k1_cosine_is_nn_cosine(ops):
    for tq, tc, d in ((129, 700, 96), (300, 129, 448)):
        q, c, _ = _designed(tq, tc, d)
        val, idx = ops.knn(q, c, 1)
        rs, ri, _, _ = ops.nn_cosine(q, c, mutual=False)
        assert torch.equal(val[..., 0], rs) and torch.equal(idx[..., 0], ri)
    x, _ = kr.planted(300, 64, 11)
    y, _ = kr.planted(700, 64, 12)
    x, y = x.to(torch.bfloat16).cuda()[None], y.to(torch.bfloat16).cuda()[None]
    val, idx = ops.knn(x, y, 1)
    rs, ri, _, _ = ops.nn_cosine(x, y, mutual=False)
    assert torch.equal(val[..., 0], rs) and torch.equal(idx[..., 0], ri)


@pytest.mark.parametrize("metric", kr.METRICS)
def test_a_problem_alone_and_inside_a_batch_gives_equal_bits(ops, metric):
    gen = torch.Generator().manual_seed(41)
    q = torch.randn(5, 300, 64, generator=gen).to(torch.bfloat16).cuda()
    c = torch.randn(5, 700, 64, generator=gen).to(torch.bfloat16).cuda()
    for k, diag in ((5, False), (16, True)):
        val, idx = ops.knn(q, c, k, metric, diag)  # 15 (pair, panel) items, another run split than one problem's 3
        v1, i1 = ops.knn(q[3:4], c[3:4], k, metric, diag)
        assert torch.equal(val[3], v1[0]) and torch.equal(idx[3], i1[0])


def test_operands_are_read_in_place(ops):
    gen = torch.Generator().manual_seed(43)
    d = 64
    buf = torch.randn(2, 129, 3 * d, generator=gen).to(torch.bfloat16).cuda()   # q | k | v side by side: the key facet, ld = 3 d
    bank = torch.randn(300, d, generator=gen).to(torch.bfloat16).cuda()
    key = buf[:, :, d:2 * d]
    want = ops.knn(key.contiguous(), bank[None].expand(2, -1, -1).contiguous(), 5, "l2")
    got = ops.knn(key, bank[None].expand(2, -1, -1), 5, "l2")                  # ld = 3 d, bank at stride 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    f32 = torch.randn(2, 129, d, generator=gen).cuda()                          # fp32: rounded once to bf16
    a, b = ops.knn(f32, bank[None].expand(2, -1, -1), 5), ops.knn(f32.to(torch.bfloat16), bank[None].expand(2, -1, -1), 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _golden(name):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    return z, kr.from_bf16_bits(z["c"]), torch.from_numpy(z["labels"]), int(z["k"])


@pytest.mark.parametrize("name", ("knn_sk_300x700x64.npz", "knn_sk_d256_k16.npz"))
def test_golden_files_sklearn_neighbours_and_predict_proba(ops, name):
    from vdr import knn
    z, c, labels, k = _golden(name)
    for metric in kr.METRICS:
        q = kr.from_bf16_bits(z["q"] if "q" in z else z[f"q_{metric}"])
        val, idx = ops.knn(q[None].cuda(), c[None].cuda(), k, metric)
        assert np.array_equal(idx[0].cpu().numpy(), z[f"idx_{metric}"]), (name, metric)
        s = kr.scores(q[None], c[None], metric)
        b = np.take_along_axis(kr.bound(q[None], c[None], s, metric), z[f"idx_{metric}"][None].astype(np.int64), -1)[0]
        want = 1.0 - z[f"dist_{metric}"] if metric == "cosine" else z[f"dist_{metric}"] ** 2
        err = np.abs(val[0].cpu().numpy().astype(np.float64) - want)
        print(f"{name} {metric}: max err / bound {(err / b).max():.3e}")
        assert (err <= b).all(), (name, metric, float((err / b).max()))
        clf = knn.KnnClassifier(c.cuda(), labels, 7, k=k, weights="uniform", metric=metric)
        proba, pred = clf.predict(q.cuda())
        assert np.array_equal(proba.cpu().numpy().astype(np.float64), z[f"proba_{metric}"].astype(np.float32).astype(np.float64))
        assert np.array_equal(pred.cpu().numpy(), z[f"pred_{metric}"])


# (queries, seed), (candidates, seed), d, k, floor of the reference's clear share: measured on the CPU 0.983 / 0.963 / 0.963,
# 0.930 / 0.907 / 0.903, 0.763 / 0.790 / 0.799 (cosine / l2 / self graph)
PLANTED = (((300, 11), (700, 12), 64, 5, 0.9), ((129, 21), (300, 22), 96, 8, 0.85), ((257, 31), (700, 32), 64, 16, 0.7))


@pytest.mark.parametrize("case", PLANTED)
def test_random_inputs_by_the_near_tie_rule(ops, case):
    (nq, sq), (nc, sc), d, k, floor = case
    q, c = kr.planted(nq, d, sq)[0][None], kr.planted(nc, d, sc)[0][None]
    for metric in kr.METRICS:
        s = kr.scores(q, c, metric)
        b = kr.bound(q, c, s, metric)
        val, idx = ops.knn(q.cuda(), c.cuda(), k, metric)
        share = kr.check_near_tie_tolerant(s, b, val.cpu().numpy(), idx.cpu().numpy(), metric, False, f"{case} {metric}")
        print(f"{case} {metric}: clear share {share:.3f}")
        assert share >= floor, (case, metric, share)
    s = kr.scores(c, c, "cosine")  # the self graph of the candidate set
    b = kr.bound(c, c, s, "cosine")
    val, idx = ops.knn(c.cuda(), c.cuda(), k, "cosine", True)
    share = kr.check_near_tie_tolerant(s, b, val.cpu().numpy(), idx.cpu().numpy(), "cosine", True, f"{case} self graph")
    print(f"{case} self graph: clear share {share:.3f}")
    assert share >= floor, (case, "self graph", share)


@pytest.mark.parametrize("metric", kr.METRICS)
def test_memory_contract(metric):
    """work exactly vdr_knn_work_bytes and outputs exactly pairs * tq * k elements between canaries: the canaries stay, every
    output element is overwritten, and stale work bytes (first NaN patterns, then the previous call's) change nothing"""
    from vdr import _lib
    lib = _lib.load()
    P, tq, tc, d, k = 3, 300, 700, 96, 9
    q, c, ref = _designed(tq, tc, d)
    s, order = ref[metric, True]
    wb = lib.vdr_knn_work_bytes(P, tq, tc, k)
    assert wb > 0 and wb % 16 == 0
    G = 4096
    w_whole, work = mg.guarded(wb, G)
    mg.fill(work, "ones")
    outs = []
    for rnd in range(2):
        v_whole, v = mg.guarded(P * tq * k * 4, G)
        i_whole, i = mg.guarded(P * tq * k * 4, G)
        _lib.check(lib.vdr_op_knn(q.data_ptr(), d, tq * d, tq, c.data_ptr(), d, tc * d, tc, P, d, k, kr.METRICS.index(metric), 1,
                                  work.data_ptr(), v.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert mg.guards_intact(w_whole, G), ("work", mg.guard_damage(w_whole, G))
        assert mg.guards_intact(v_whole, G) and mg.guards_intact(i_whole, G)
        val, idx = v.view(torch.float32).view(P, tq, k), i.view(torch.int32).view(P, tq, k)
        assert mg.canary_left(val) == 0 and mg.canary_left(idx) == 0
        _exact((val, idx), s, order, k, P, (metric, "guarded", rnd))
        outs.append((val.clone(), idx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_search_chunks_and_classifier_on_the_device(ops):
    from vdr import knn
    q, c, _ = _designed(129, 700, 96)
    for metric, diag in (("cosine", False), ("l2", True)):
        want = ops.knn(q, c, 8, metric, diag)
        got = knn.search(q, c, 8, metric=metric, exclude_diag=diag, bank_chunk=129)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    x, _ = kr.planted(300, 64, 12)
    v, i = knn.graph(x.cuda(), 5)
    w = ops.knn(x[None].cuda(), x[None].cuda(), 5, "cosine", True)
    assert torch.equal(v, w[0][0]) and torch.equal(i, w[1][0])


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_knn_tiny") as m:
        yield m


def test_model_transfer_labels_fit_knn_and_memory_bank(ops, model):
    import vdr
    from vdr import anomaly, knn
    x1, x2 = vo.make_images(TINY, 2, seed=6).cuda(), vo.make_images(TINY, 2, seed=9).cuda()
    gh, gw = model.grid
    t = gh * gw
    labels = torch.randint(0, 4, (2, gh, gw), generator=torch.Generator().manual_seed(3))
    p = model.transfer_labels(x1, labels, x2, 4, k=5, temperature=0.1)
    (desc,), _, _ = model.engine.forward_descriptors(torch.cat([x2, x1]), [vdr.FacetOut(TINY.layers - 1, "key", 0, False, torch.bfloat16)],
                                                     maps=[])
    val, idx = ops.knn(desc[:2], desc[2:], 5)
    scores = knn.vote(idx, val, labels.cuda().reshape(2, t), 4, weights="softmax", temperature=0.1)
    assert p.radius is None and p.grid == (gh, gw) and torch.equal(p.idx, idx) and torch.equal(p.val, val)
    assert torch.equal(p.scores, scores.reshape(2, gh, gw, 4)) and torch.equal(p.labels, knn.lowest_argmax(scores).reshape(2, gh, gw))
    with pytest.raises(ValueError, match="at most 16"):
        model.transfer_labels(x1, labels, x2, 4, k=17)
    # a two-class toy bank: the classifier is search + vote on linear_probe_features, rows in batch order
    batches = [x1, x2]
    y = torch.tensor([0, 1, 1, 0])
    clf = model.fit_knn(batches, y, 2, k=3, temperature=0.07)
    feats = torch.cat([model.linear_probe_features(b, 1, False) for b in batches])
    assert torch.equal(clf.features, feats.to(torch.bfloat16)) and clf.k == 3
    got_scores, got_labels = model.knn_predict(x2, clf)
    v, i = ops.knn(feats[None, 2:], feats[None].to(torch.bfloat16), 3)
    want = knn.vote(i[0], v[0], y.cuda(), 2, weights="softmax", temperature=0.07)
    assert torch.equal(got_scores, want) and torch.equal(got_labels, knn.lowest_argmax(want))
    assert tuple(got_scores.shape) == (2, 2) and torch.allclose(got_scores.sum(-1), torch.ones(2, device="cuda"), atol=1e-6)
    # MemoryBank: the default keeps nn_cosine's bits, k = 1 is the default, k = 3 the mean of the three smallest distances
    gen = torch.Generator().manual_seed(5)
    xb = torch.randn((3, 50, 64), generator=gen).cuda().to(torch.bfloat16)
    bank = anomaly.MemoryBank(xb.reshape(150, 64)[::7])
    base = 1.0 - ops.nn_cosine(xb, bank.bank.unsqueeze(0).expand(3, -1, -1), mutual=False)[0]
    assert torch.equal(bank.score(xb), base) and torch.equal(bank.score(xb, k=1), base)
    d3 = 1.0 - ops.knn(xb, bank.bank.unsqueeze(0).expand(3, -1, -1), 3)[0]
    assert torch.equal(bank.score(xb, k=3), ((d3[..., 0] + d3[..., 1]) + d3[..., 2]) / 3.0) and torch.equal(d3[..., 0], base)
    rw = bank.score(xb, k=3, reweight=True)
    assert torch.equal(rw, (1.0 - torch.softmax(d3, -1)[..., 0]) * d3[..., 0]) and bool((rw <= base + 1e-7).all())
