"""GPU: vdr_op_kmeans_assign / vdr_op_kmeans_update (csrc/kmeans.hip) at op level and vdr.kmeans.fit against the restatement of
their definitions (tests/kmeans_ref.py) and against scikit-learn (tests/golden/kmeans_sk_*.npz, README_kmeans.md).

Designed inputs (x integer in [-4, 4], centroids multiples of 2^-8: hi + lo is exact, every partial sum of the MFMAs is exact
in fp32) must come back bit for bit in every output: labels, min_dist, inertia, the changed count, the centroids (one IEEE
division) and the counts; duplicate centroids resolve to the lowest index, a centroid no row chooses keeps its bits.  X and
the centroids are drawn differently, so a row / column swap of the accumulator layout shows.  Cases (R, k, d, imgs) cover
rows 1, 127, 128, 129, 257 (ragged panels, more than one), VDR_KMEANS_CHUNK - 1, the chunk, the chunk + 1 and twice the chunk
+ 1, k in {1, 2, 127, 128, 129, 257, 1024} (ragged centroid tiles, up to eight), d in {32, 64, 96, 416} (half a step, one
step, a short last step, 6.5 steps) and a joint problem of 3 images.
Random bf16 maps are held to the restatement's bounds; labels must be equal wherever the float64 margin exceeds the label
bound, which may leave out at most 1 % of the rows (asserted on the restatement alone)."""
import os
import warnings

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

CH = kr.KMEANS_CHUNK
#        R            k     d   imgs
CASES = ((1,          1,    32,  1),
         (127,        2,    64,  1),
         (128,        127,  96,  1),
         (129,        128,  416, 1),
         (257,        129,  32,  1),
         (CH - 1,     2,    96,  1),
         (CH,         128,  64,  1),
         (CH + 1,     257,  64,  1),
         (2 * CH + 1, 129,  416, 1),
         (1100,       1024, 32,  1),
         (129,        5,    96,  3))
GOLDENS = ("kmeans_sk_130x32", "kmeans_sk_333x96", "kmeans_sk_520x416")
INERTIA_GATE = 4 * 1.42e-7  # README_kmeans.md: four times the worst relative distance the fp32 emulation measures against sklearn


@pytest.fixture(scope="module")
def kmeans():
    from vdr import kmeans
    return kmeans


_CACHE = {}


def _designed(R, k, d):
    """two problems: (x [2, R, d], c [2, k, d], prev labels, the fp32-emulated assignment and update of each) -- computed once
    per case, shared, never written"""
    key = ("designed", R, k, d)
    if key not in _CACHE:
        xs, cs, prevs, As, Us = [], [], [], [], []
        for p in range(2):
            x, c = kr.designed(R, k, d, seed=100000 * p + 1000 * R + 10 * k + d)
            prev = np.zeros(R, np.int32)  # (the rows not labelled 0 count as changed)
            a = kr.assign_fp32(x, c, prev)
            xs.append(x), cs.append(c), prevs.append(prev), As.append(a), Us.append(kr.update_fp32(x, a["labels"], c))
        _CACHE[key] = (np.stack(xs), np.stack(cs), np.stack(prevs), As, Us)
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "R{}_k{}_d{}_imgs{}".format(*c))
def test_designed_inputs_are_exact(ops, case):
    R, k, d, imgs = case
    x, c, prev, As, Us = _designed(R, k, d)
    if k >= 5:  # (something to see: duplicate centroids, a centroid without rows)
        assert all((u[1] == 0).any() for u in Us) and all((a["labels"] != 3).all() and (a["labels"] != k - 1).all() for a in As)
    t = R // imgs
    assert t * imgs == R
    xg = torch.from_numpy(x).cuda().to(torch.bfloat16)
    cg = torch.from_numpy(c).cuda()
    if imgs > 1:  # two joint problems of `imgs` images each
        xg = xg.reshape(2, imgs, t, d)
    labels = torch.from_numpy(prev).cuda().clone()
    lab, md, inertia, changed = ops.kmeans_assign(xg, cg, labels)
    cent, counts = ops.kmeans_update(xg, lab, cg)
    torch.cuda.synchronize()
    assert lab.dtype == torch.int32 and counts.dtype == torch.int32 and changed.dtype == torch.int32
    for p in range(2):
        a, (uc, un) = As[p], Us[p]
        got = lab[p].cpu().numpy()
        assert np.array_equal(got, a["labels"]), (p, "labels", np.argwhere(got != a["labels"])[:4].tolist())
        assert np.array_equal(_bits(md[p].cpu().numpy()), _bits(a["min_dist"])), (p, "min_dist")
        assert _bits(inertia[p:p + 1].cpu().numpy())[0] == _bits(a["inertia"])[()], (p, "inertia", float(inertia[p]), float(a["inertia"]))
        assert int(changed[p]) == a["changed"], (p, "changed")
        assert np.array_equal(counts[p].cpu().numpy(), un), (p, "counts")
        assert np.array_equal(_bits(cent[p].cpu().numpy()), _bits(uc)), (p, "centroids", np.argwhere(_bits(cent[p].cpu().numpy()) != _bits(uc))[:4].tolist())
    assert np.array_equal(_bits(cg.cpu().numpy()), _bits(c))  # (inplace=False: the input is not written)


def test_views_and_batches_give_the_contiguous_bits(ops):
    P, t, k, d = 3, 200, 5, 64
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(P, t, d, generator=gen).to(torch.bfloat16).cuda()
    c = (torch.randn(P, k, d, generator=gen) * 0.7).cuda()

    def run(xv, cv):
        lab, md, inertia, changed = ops.kmeans_assign(xv, cv)
        cent, counts = ops.kmeans_update(xv, lab, cv)
        return [v.clone() for v in (lab, md, inertia, changed, cent, counts)]

    want = run(x, c)
    wide = torch.randn(P, t, 3 * d, generator=gen).to(torch.bfloat16).cuda()
    wide[:, :, d:2 * d] = x
    view = wide[:, :, d:2 * d]
    assert ops.kmeans_operand(view).x.data_ptr() == view.data_ptr()  # (read in place)
    tall = torch.randn(P, t + 5, d, generator=gen).to(torch.bfloat16).cuda()
    tall[:, 5:] = x
    assert ops.kmeans_operand(tall[:, 5:]).x.data_ptr() == tall[:, 5:].data_ptr()
    for what, got in (("column slice", run(view, c)), ("row prefix", run(tall[:, 5:], c))):
        for g, w in zip(got, want):
            assert torch.equal(g, w), what
    # a problem's bits are those of its one-problem run; a problem stride of 0 is the same map under three sets of centroids
    for p in range(P):
        for g, w in zip(run(x[p:p + 1], c[p:p + 1]), want):
            assert torch.equal(g[0], w[p]), ("single", p)
    shared = x[1:2].expand(P, t, d)
    assert ops.kmeans_operand(shared).problem_stride == 0
    got = run(shared, c)
    for p in range(P):
        for g, w in zip(got, run(x[1:2], c[p:p + 1])):
            assert torch.equal(g[p], w[0]), ("stride 0", p)
    # an inactive problem is not touched
    active = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    lab = torch.full((P, t), -7, dtype=torch.int32).cuda()
    out = (torch.full((P, t), -1.0).cuda(), torch.full((P,), -1.0).cuda(), torch.full((P,), -5, dtype=torch.int32).cuda())
    ops.kmeans_assign(x, c, lab, active=active, out=out)
    cent, counts = ops.kmeans_update(x, lab, c, active=active, counts=torch.full((P, k), -3, dtype=torch.int32).cuda())
    assert (lab[1] == -7).all() and (out[0][1] == -1).all() and float(out[1][1]) == -1 and int(out[2][1]) == -5
    assert torch.equal(cent[1], c[1]) and (counts[1] == -3).all()
    for p in (0, 2):
        assert torch.equal(lab[p], want[0][p]) and torch.equal(out[0][p], want[1][p]) and torch.equal(cent[p], want[4][p])
        assert int(out[2][p]) == t


def _random(R, k, d, seed):
    key = ("random", R, k, d)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(R, d, generator=gen).to(torch.bfloat16).float().numpy()
        c = (x[:k] * 0.75 + 0.2 * torch.randn(k, d, generator=gen).numpy()).astype(np.float32)
        a = kr.assign(x, c)
        lb, mdb, ib = kr.assign_bounds(x, c, a)
        _CACHE[key] = (x, c, a, lb, mdb, ib)
    return _CACHE[key]


@pytest.mark.parametrize("shape", ((300, 16, 96, 3), (300, 16, 416, 4), (200, 130, 768, 5)), ids=lambda s: "R{}_k{}_d{}".format(*s[:3]))
def test_random_maps_stay_inside_the_bounds(ops, shape):
    R, k, d, seed = shape
    x, c, a, lb, mdb, ib = _random(R, k, d, seed)
    clear = a["margin"] > lb
    print(f"rows under the label bound: {(~clear).mean():.4f}")
    assert (~clear).mean() <= 0.01  # a condition of the test, on the restatement alone
    xg = torch.from_numpy(x).cuda().to(torch.bfloat16).unsqueeze(0)
    cg = torch.from_numpy(c).cuda().unsqueeze(0)
    lab, md, inertia, changed = ops.kmeans_assign(xg, cg)
    cent, counts = ops.kmeans_update(xg, lab, cg)
    lab_n = lab[0].cpu().numpy()
    assert lab_n.min() >= 0 and lab_n.max() < k and int(changed[0]) == R
    assert np.array_equal(lab_n[clear], a["labels"][clear])
    h_got = np.take_along_axis(a["h"], lab_n.astype(np.int64)[:, None], 1)[:, 0]
    xx = (x.astype(np.float64) ** 2).sum(-1)
    err = np.abs(md[0].cpu().numpy().astype(np.float64) - np.maximum(xx + h_got, 0.0))
    print(f"max |min_dist - restatement| {err.max():.3e}, bound {mdb.min():.3e} .. {mdb.max():.3e}")
    same = lab_n == a["labels"]
    assert (err[same] <= mdb[same]).all()
    assert (err[~same] <= (mdb + lb)[~same]).all()
    if same.all():
        assert abs(float(inertia[0]) - a["inertia"]) <= ib
    want_c, want_n = kr.update(x, lab_n, c)
    assert np.array_equal(counts[0].cpu().numpy(), want_n)
    cerr = np.abs(cent[0].cpu().numpy().astype(np.float64) - want_c)
    cb = kr.centroid_bound(x, lab_n, want_c) + kr.U * np.abs(want_c)  # (+ the restatement's own rounding of the mean to fp32)
    print(f"max |centroid - restatement| {cerr.max():.3e}, bound up to {cb.max():.3e}")
    assert (cerr <= cb).all()


def _golden(golden_dir, name):
    key = ("golden", name)
    if key not in _CACHE:
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        _CACHE[key] = {f: z[f] for f in z.files}
        _CACHE[key]["x"] = kr.from_bf16_bits(z["x_bits"])
    return _CACHE[key]


@pytest.mark.parametrize("name", GOLDENS)
def test_fit_reproduces_sklearn_on_the_goldens(kmeans, golden_dir, name):
    z = _golden(golden_dir, name)
    x = torch.from_numpy(z["x"]).cuda()
    init = torch.from_numpy(z["init"]).cuda().unsqueeze(0)
    k = init.shape[1]
    res = kmeans.fit(x, k, init=init)
    assert bool(res.converged[0]) and int(res.iters[0]) == int(z["ref_iters"]) == int(z["sk_n_iter"])
    lab = res.labels[0].cpu().numpy()
    assert np.array_equal(lab, z["sk_labels"])
    cerr = np.abs(res.centroids[0].cpu().numpy().astype(np.float64) - z["sk_centers"])
    cb = kr.centroid_bound(z["x"], lab, z["sk_centers"])
    print(f"{name}: max |centroid - sklearn| {cerr.max():.3e}, min slack {(cb - cerr).min():.3e}")
    assert (cerr <= cb).all()
    rel = abs(float(res.inertia[0]) - float(z["sk_inertia"])) / float(z["sk_inertia"])
    print(f"{name}: inertia relative to sklearn {rel:.3e} (gate {INERTIA_GATE:.1e})")
    assert rel <= INERTIA_GATE
    assert np.array_equal(res.counts[0].cpu().numpy(), np.bincount(z["sk_labels"], minlength=k))
    # the flags are never read with sync_every=0: the same bits
    res0 = kmeans.fit(x, k, init=init, sync_every=0)
    for f in ("labels", "centroids", "inertia", "counts", "iters", "converged"):
        assert torch.equal(getattr(res0, f), getattr(res, f)), f


def test_restarts_return_the_best_single_restart(kmeans, golden_dir):
    z = _golden(golden_dir, GOLDENS[0])
    x = torch.from_numpy(z["x"]).cuda()
    R, k = x.shape[0], 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = kmeans.fit(x, k, init="random", n_init=4, seed=5)
    gen = torch.Generator().manual_seed(5)
    singles = [kmeans.fit(x, k, init=x[torch.randperm(R, generator=gen)[:k].cuda()].unsqueeze(0)) for _ in range(4)]
    inertia = [float(s.inertia[0]) for s in singles]
    best = singles[inertia.index(min(inertia))]
    assert len(set(inertia)) > 1  # (the restarts differ: there is a choice to make)
    for f in ("labels", "centroids", "inertia", "counts", "iters", "converged"):
        assert torch.equal(getattr(res, f), getattr(best, f)), f


def test_max_iter_warns_and_reports(kmeans, golden_dir):
    z = _golden(golden_dir, GOLDENS[1])
    x = torch.from_numpy(z["x"]).cuda()
    init = torch.from_numpy(z["init"]).cuda().unsqueeze(0)
    with pytest.warns(kmeans.ConvergenceWarning) as rec:
        res = kmeans.fit(x, init.shape[1], init=init, max_iter=2)
    assert len(rec) == 1
    assert not bool(res.converged[0]) and int(res.iters[0]) == 2
    # the centroids are the means of the labels returned
    want_c, want_n = kr.update(z["x"], res.labels[0].cpu().numpy(), z["init"])
    assert np.array_equal(res.counts[0].cpu().numpy(), want_n)
    assert (np.abs(res.centroids[0].cpu().numpy() - want_c) <= kr.centroid_bound(z["x"], res.labels[0].cpu().numpy(), want_c) + kr.U * np.abs(want_c)).all()
