"""CPU: the k-NN statement (tests/knn_ref.py) against scikit-learn's golden answers, its fp32 bounds and its acceptance rule
against an fp32 evaluation in another summation order, and vdr.knn.vote on CPU tensors against sklearn's predict_proba."""
import os

import numpy as np
import pytest
import torch

import knn_ref as kref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def _cases():
    """(file, metric, q, c, labels, k, golden dict)"""
    g1, g2 = _golden("knn_sk_300x700x64.npz"), _golden("knn_sk_d256_k16.npz")
    for m in kref.METRICS:
        yield "300x700x64", m, kref.from_bf16_bits(g1["q"]), kref.from_bf16_bits(g1["c"]), g1["labels"], int(g1["k"]), g1
        yield "d256_k16", m, kref.from_bf16_bits(g2[f"q_{m}"]), kref.from_bf16_bits(g2["c"]), g2["labels"], int(g2["k"]), g2


CASES = list(_cases())
IDS = [f"{c[0]}-{c[1]}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_sklearn_on_the_golden_files(case):
    name, m, q, c, _, k, g = case
    s = kref.scores(q[None], c[None], m)
    val, idx = kref.topk(s, k, m)
    assert np.array_equal(idx[0], g[f"idx_{m}"])
    dist = np.sqrt(val[0]) if m == "l2" else 1.0 - val[0]
    err = np.abs(dist - g[f"dist_{m}"]).max()
    print(f"{name} {m}: max |dist - sklearn| {err:.3e}")
    assert err <= 1e-9 * max(1.0, float(np.abs(dist).max()))
    # every stored row is a clear one: the generator's filter, restated
    assert kref.clear_rows(s, kref.bound(q[None], c[None], s, m), k, m).all()


@pytest.mark.parametrize("metric", kref.METRICS)
@pytest.mark.parametrize("d", (32, 96, 448, 768))
def test_an_fp32_evaluation_in_another_order_stays_under_the_bound(d, metric):
    q, _ = kref.planted(130, d, seed=3 + d)
    c, _ = kref.planted(257, d, seed=4 + d)
    q, c = q[None], c[None]
    s = kref.scores(q, c, metric)
    b = kref.bound(q, c, s, metric)
    ratio = np.abs(kref.fp32_other_order(q, c, metric).astype(np.float64) - s) / b
    print(f"{metric} d={d}: max err / bound {ratio.max():.4f}, max bound {b.max():.3e}")
    assert ratio.max() < 1.0
    # designed inputs need no bound: every fp32 evaluation IS the float64 one
    import nn_cosine_ref as nref
    x, y = nref.designed(1, 40, 50, d, seed=d)
    assert np.array_equal(kref.fp32_other_order(x, y, metric).astype(np.float64), kref.scores(x, y, metric))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vote_on_cpu_tensors_equals_sklearn(case):
    import vdr
    _, m, q, c, labels, k, g = case
    idx = torch.from_numpy(g[f"idx_{m}"])
    val = torch.from_numpy(kref.topk(kref.scores(q[None], c[None], m), k, m)[0][0]).float()
    want = g[f"proba_{m}"]
    n_classes = want.shape[1]
    got = vdr.knn.vote(idx, val, torch.from_numpy(labels), n_classes, weights="uniform", metric=m)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert np.array_equal(vdr.knn.lowest_argmax(got).numpy(), g[f"pred_{m}"])  # (the planted labels are 0..6: class id == column)
    # the softmax vote: a distribution per query, deterministic, equivariant under a permutation of the class ids
    soft = vdr.knn.vote(idx, val, torch.from_numpy(labels), n_classes, metric=m)
    assert torch.allclose(soft.sum(-1), torch.ones(soft.shape[0]), atol=1e-6)
    assert torch.equal(soft, vdr.knn.vote(idx, val, torch.from_numpy(labels), n_classes, metric=m))
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4])
    assert torch.equal(vdr.knn.vote(idx, val, perm[torch.from_numpy(labels)], n_classes, metric=m)[:, perm], soft)
    sim = val.double() if m == "cosine" else -val.double().sqrt()
    w = torch.softmax(sim / 0.07, -1)
    ref = torch.zeros(soft.shape, dtype=torch.float64)
    near = torch.from_numpy(labels)[idx.long()]
    for j in range(k):
        ref[torch.arange(ref.shape[0]), near[:, j]] += w[:, j]
    assert (soft.double() - ref).abs().max() < 1e-5


def test_uniform_vote_is_one_correctly_rounded_division():
    """count / k in fp32 equals sklearn's float64 count / k rounded to fp32, for every count <= k <= 16"""
    for k in range(1, 17):
        for n in range(k + 1):
            assert np.float32(n) / np.float32(k) == np.float32(np.float64(n) / np.float64(k)), (n, k)


def test_the_predicted_class_is_the_lowest_on_a_tie():
    import vdr
    labels = torch.tensor([1, 0, 0, 2])
    idx = torch.tensor([[0, 1], [3, 0], [2, 1]])
    scores = vdr.knn.vote(idx, torch.ones(3, 2), labels, 3, weights="uniform")
    assert scores.tolist() == [[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [1.0, 0.0, 0.0]]
    assert vdr.knn.lowest_argmax(scores).tolist() == [0, 1, 0]


def test_labels_broadcast_over_leading_dimensions_and_per_problem_labels():
    import vdr
    gen = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 50, (4, 9, 5), generator=gen)
    val = torch.rand(4, 9, 5, generator=gen)
    shared = torch.randint(0, 6, (50,), generator=gen)
    per = torch.randint(0, 6, (4, 50), generator=gen)
    for w in ("softmax", "uniform"):
        all4 = vdr.knn.vote(idx, val, shared, 6, weights=w)
        mine = vdr.knn.vote(idx, val, per, 6, weights=w)
        assert tuple(all4.shape) == (4, 9, 6)
        for p in range(4):  # a problem's scores do not depend on the batch
            assert torch.equal(all4[p], vdr.knn.vote(idx[p], val[p], shared, 6, weights=w))
            assert torch.equal(mine[p], vdr.knn.vote(idx[p], val[p], per[p], 6, weights=w))
    # l2 votes with -sqrt(val): a nearer neighbour weighs more, and the temperature sharpens
    one = vdr.knn.vote(torch.tensor([[0, 1]]), torch.tensor([[1.0, 4.0]]), torch.tensor([0, 1]), 2, metric="l2", temperature=1.0)
    want = torch.softmax(torch.tensor([-1.0, -2.0]), 0)
    assert torch.allclose(one[0], want, atol=1e-7)
    sharp = vdr.knn.vote(torch.tensor([[0, 1]]), torch.tensor([[1.0, 4.0]]), torch.tensor([0, 1]), 2, metric="l2", temperature=0.1)
    assert sharp[0, 0] > one[0, 0]


@pytest.mark.parametrize("metric", kref.METRICS)
def test_the_acceptance_rule_on_an_fp32_evaluation(metric):
    """the rule a kernel's random-input test applies, run here on the fp32 emulation: it passes, and the exact-order part is
    not vacuous (the float64 reference alone clears 0.96 of these rows)"""
    q, _ = kref.planted(300, 64, seed=100)
    c, _ = kref.planted(700, 64, seed=200)
    q, c = q[None], c[None]
    s = kref.scores(q, c, metric)
    b = kref.bound(q, c, s, metric)
    f = kref.fp32_other_order(q, c, metric)
    order = np.argsort(kref.cost(f, metric), axis=-1, kind="stable")[..., :5]
    clear = kref.check_near_tie_tolerant(s, b, np.take_along_axis(f, order, -1), order.astype(np.int32), metric, what=f"fp32 {metric}")
    print(f"{metric}: clear rows {clear:.3f}")
    assert clear >= 0.9
    # ... and it does reject a wrong answer: two neighbours exchanged on a clear row
    bad = order.astype(np.int32).copy()
    row = int(np.flatnonzero(kref.clear_rows(s, b, 5, metric)[0])[0])
    bad[0, row, [0, 1]] = bad[0, row, [1, 0]]
    with pytest.raises(AssertionError):
        kref.check_near_tie_tolerant(s, b, np.take_along_axis(f, bad.astype(np.int64), -1), bad, metric)
    # the self graph leaves the diagonal out
    s2 = kref.scores(c[:, :300], c[:, :300], metric)
    _, i2 = kref.topk(s2, 16, metric, exclude_self=True)
    assert (i2 != np.arange(300).reshape(1, 300, 1)).all()
    _, i1 = kref.topk(s2, 1, metric)
    assert (i1[0, :, 0] == np.arange(300)).all()


def test_vote_refuses_bad_arguments():
    import vdr
    idx, val, labels = torch.zeros(4, 3, dtype=torch.long), torch.zeros(4, 3), torch.zeros(8, dtype=torch.long)
    with pytest.raises(ValueError, match="weights"):
        vdr.knn.vote(idx, val, labels, 2, weights="distance")
    with pytest.raises(ValueError, match="metric"):
        vdr.knn.vote(idx, val, labels, 2, metric="euclidean")
    with pytest.raises(ValueError, match="one shape"):
        vdr.knn.vote(idx, val[:, :2], labels, 2)
    with pytest.raises(TypeError, match="idx"):
        vdr.knn.vote(val, val, labels, 2)
    with pytest.raises(TypeError, match="labels"):
        vdr.knn.vote(idx, val, labels.float(), 2)
    with pytest.raises(ValueError, match="leading dimensions"):
        vdr.knn.vote(idx, val, torch.zeros(2, 2, 8, dtype=torch.long), 2)
    with pytest.raises(ValueError, match="n_classes"):
        vdr.knn.vote(idx, val, labels, 0)
    with pytest.raises(ValueError, match="temperature"):
        vdr.knn.vote(idx, val, labels, 2, temperature=0.0)
