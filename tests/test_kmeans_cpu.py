"""CPU: the float64 restatement of the k-means definitions (tests/kmeans_ref.py) against scikit-learn's recorded fits
(tests/golden/kmeans_sk_*.npz, README_kmeans.md) and its own bounds; every C-ABI refusal of vdr_op_kmeans_assign /
vdr_op_kmeans_update returns its code before a device is touched, and without a GPU both fail loudly; vdr.kmeans.vote and
maximin on hand-made arrays, ties included; the selection logic of Correspondences.points(select="kmeans") with a stubbed
fit; the Python refusals of fit, cosegment and points; points(select="similarity") and a Correspondences built positionally
behave as before."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from fixtures import lib  # noqa: F401

GOLDENS = ("kmeans_sk_130x32", "kmeans_sk_333x96", "kmeans_sk_520x416")
INERTIA_WORST = 1.42e-7  # README_kmeans.md: the worst relative distance of the fp32 emulation's inertia from sklearn's


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_sklearn(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    x = kr.from_bf16_bits(z["x_bits"])
    R, d = (int(v) for v in name.split("_")[-1].split("x"))
    assert x.shape == (R, d) and z["x_bits"].dtype == np.uint16 and os.path.getsize(os.path.join(golden_dir, name + ".npz")) <= 840636
    worst = [np.inf]

    def step(it, a, c):
        worst[0] = min(worst[0], float((a["margin"] / kr.assign_bounds(x, c, a)[0]).min()))

    ref = kr.lloyd(x, z["init"], 300, step)
    assert ref["converged"] and ref["iters"] == int(z["ref_iters"]) == int(z["sk_n_iter"]) >= 10
    assert worst[0] > 4.0  # (the generator's condition: no fp32 evaluation can label a row differently)
    assert np.array_equal(ref["labels"], z["sk_labels"])
    assert (ref["counts"] > 0).all()
    # centres: the restatement rounds the float64 mean to fp32, sklearn keeps float64 (it agrees with the float64 mean to 5e-15)
    assert (np.abs(ref["centroids"] - z["sk_centers"]) <= kr.U * np.abs(z["sk_centers"]) + 1e-13).all()
    assert abs(ref["inertia"] - float(z["sk_inertia"])) / float(z["sk_inertia"]) <= 1e-7
    emu = kr.lloyd_fp32(x, z["init"], 300)
    assert np.array_equal(emu["labels"], z["sk_labels"]) and emu["iters"] == ref["iters"]
    rel = abs(float(emu["inertia"]) - float(z["sk_inertia"])) / float(z["sk_inertia"])
    print(f"{name}: fp32 emulation's inertia relative to sklearn {rel:.3e}")
    assert rel <= INERTIA_WORST
    assert (np.abs(emu["centroids"].astype(np.float64) - z["sk_centers"]) <= kr.centroid_bound(x, emu["labels"], z["sk_centers"])).all()


@pytest.mark.parametrize("shape", ((150, 9, 32), (150, 9, 416), (64, 40, 768)))
def test_an_fp32_evaluation_in_another_order_stays_inside_the_bounds(shape):
    R, k, d = shape
    rng = np.random.default_rng(R + k + d)
    x = kr.bf16_rn(rng.normal(size=(R, d))).astype(np.float32)
    c = (x[:k] * 0.5 + 0.3 * rng.normal(size=(k, d))).astype(np.float32)
    a = kr.assign(x, c)
    hb = kr.h_bound(x, c, a["h"])
    hi, lo = kr.split(c)
    # fp32 throughout, channels in DESCENDING order, hi and lo in separate accumulators: not the kernel's order
    s = np.zeros((R, k), np.float32)
    s2 = np.zeros((R, k), np.float32)
    for ch in range(d - 1, -1, -1):
        s = (s + x[:, ch:ch + 1] * hi[:, ch].astype(np.float32)[None, :]).astype(np.float32)
        s2 = (s2 + x[:, ch:ch + 1] * lo[:, ch].astype(np.float32)[None, :]).astype(np.float32)
    cc = (c * c).sum(-1, dtype=np.float32)
    h = (cc[None, :] - np.float32(2) * (s + s2).astype(np.float32)).astype(np.float32)
    ratio = np.abs(h.astype(np.float64) - a["h"]) / hb
    print(f"d = {d}: worst |h32 - h64| / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # the split leaves 2^-17 of the centroid: s against the dot product with the fp32 centroid itself
    full = x.astype(np.float64) @ c.astype(np.float64).T
    assert (np.abs(kr.scores(x, c)[3] - full) <= kr.split_residual_bound(x, c)).all()
    # designed inputs: the emulation is the float64 result exactly
    xd, cd = kr.designed(70, 6, d, 3)
    ad, ed = kr.assign(xd, cd), kr.assign_fp32(xd, cd)
    assert np.array_equal(ad["labels"], ed["labels"]) and (ad["labels"] != 3).all() and (ad["labels"] != 5).all() and (ad["labels"] != 2).all()
    hi, lo = kr.split(cd)
    assert np.array_equal(hi + lo, cd.astype(np.float64))
    assert np.array_equal(kr.sumsq_lanes(xd).astype(np.float64), (xd.astype(np.float64) ** 2).sum(-1))


def test_fixed_order_sums():
    v = np.arange(1, 2051, dtype=np.float32)  # exact in any order
    assert float(kr.sum_colmean_order(v)) == 2050 * 2051 / 2
    big = np.float32(2.0 ** 24)
    v = np.zeros(32, np.float32)
    v[0], v[16] = big, 1.0  # rows 0 and 16 share interleaved sum 0: 2^24 + 1 rounds back to 2^24
    assert float(kr.sum_colmean_order(v)) == 2.0 ** 24
    v[16], v[17] = 0.0, 1.0
    v[1] = 1.0  # lane 1 holds 2 exactly; folded into lane 0: 2^24 + 2 is representable
    assert float(kr.sum_colmean_order(v)) == 2.0 ** 24 + 2


def _aligned(n=4096):
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) & ~15


def _assign_args(p, **kw):
    #        x, ld, image_stride, problem_stride, problems, imgs, t, d, k, centroids, active, work, labels, min_dist, inertia, changed, stream
    a = dict(x=p, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, k=3, centroids=p, active=None,
             work=p, labels=p, min_dist=p, inertia=p, changed=p, stream=None)
    a.update(kw)
    return list(a.values())


def _update_args(p, **kw):
    #        x, ld, image_stride, problem_stride, problems, imgs, t, d, k, labels, active, work, centroids, counts, stream
    a = dict(x=p, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, k=3, labels=p, active=None, work=p,
             centroids=p, counts=p, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("op", ("assign", "update"))
def test_ops_refuse_bad_arguments_before_touching_a_device(lib, op):
    keep, p = _aligned()
    fn, args = (lib.vdr_op_kmeans_assign, _assign_args) if op == "assign" else (lib.vdr_op_kmeans_update, _update_args)
    INVALID, UNSUPPORTED = -1, -7
    ptrs = ("x", "centroids", "work", "labels", "min_dist", "inertia", "changed") if op == "assign" else \
        ("x", "labels", "work", "centroids", "counts")
    for name in ptrs:
        assert fn(*args(p, **{name: None})) == INVALID, name
        assert b"null" in lib.vdr_last_error(None)
        assert fn(*args(p, **{name: p + 4})) == INVALID, name  # misaligned
        assert b"aligned" in lib.vdr_last_error(None)
    assert fn(*args(p, active=p + 8)) == INVALID
    for name in ("problems", "imgs", "t", "d"):
        for v in (0, -1):
            assert fn(*args(p, **{name: v})) == INVALID, (name, v)
    for d in (8, 48, 100):
        assert fn(*args(p, d=d, ld=128)) == UNSUPPORTED, d
        assert b"multiple of 32" in lib.vdr_last_error(None)
    for k in (0, -3, 1025, 5000):
        assert fn(*args(p, k=k, t=4096)) == UNSUPPORTED, k
        assert b"1..1024" in lib.vdr_last_error(None)
    assert fn(*args(p, k=21)) == INVALID  # k > R = 20
    assert b"rows" in lib.vdr_last_error(None)
    assert fn(*args(p, ld=56)) == INVALID  # ld < d
    for name in ("image_stride", "problem_stride"):
        assert fn(*args(p, **{name: -8})) == INVALID, name
        assert fn(*args(p, **{name: 12})) == INVALID, name  # not a multiple of 8 elements
    assert fn(*args(p, ld=68)) == INVALID
    assert fn(*args(p, problems=2 ** 20, imgs=2 ** 6, t=2 ** 5)) == INVALID  # problems * R = 2^31
    assert b"2^31" in lib.vdr_last_error(None)
    assert lib.vdr_kmeans_work_bytes(0, 1, 1, 32, 1) == 0
    n = lib.vdr_kmeans_work_bytes(2, 2, 10, 64, 3)
    assert n >= 4 * max(2 * 2 * 20 + 2 * 3, 2 * 1 * 3 * 64) and n % 16 == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_loud_failure_not_fallback(lib):
    keep, p = _aligned()
    assert lib.vdr_op_kmeans_assign(*_assign_args(p)) == -2  # VDR_ERR_NO_DEVICE
    assert b"no CPU path" in lib.vdr_last_error(None)
    assert lib.vdr_op_kmeans_update(*_update_args(p)) == -2
    from vdr import kmeans, ops
    with pytest.raises(TypeError, match="HIP device"):
        ops.kmeans_assign(torch.zeros(1, 4, 32), torch.zeros(1, 2, 32))
    with pytest.raises(TypeError, match="HIP device"):
        kmeans.fit(torch.zeros(1, 4, 32), 2)


def test_constants_follow_the_header():
    import re
    from vdr import ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdr.h")).read()
    chunk = int(re.search(r"#define VDR_KMEANS_CHUNK (\d+)", hdr).group(1))
    assert chunk == ops.KMEANS_CHUNK == kr.KMEANS_CHUNK
    assert int(re.search(r"#define VDR_COV_CHUNK (\d+)", hdr).group(1)) == kr.COV_CHUNK


def test_vote_on_hand_made_arrays():
    from vdr import kmeans
    labels = torch.tensor([[0, 0, 1, 1, 2, 2], [0, 1, 1, 1, 1, 1], [0, 0, 0, 2, 2, 2], [3, 3, 3, 3, 3, 3]])
    sal = torch.tensor([[0.9, 0.1, 0.25, 0.25, 0.0, 0.0],  # cluster 0: mean 0.5 yes; 1: 0.25 yes; 2: 0 no
                        [0.3, 0.9, 0.9, 0.9, 0.9, 0.9],    # 0: yes; 1: yes; 2: no patch -> no
                        [0.25, 0.25, 0.25, 0.5, 0.5, 0.5],  # 0: 0.25 yes; 2: yes
                        [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])   # 3: yes; no patch elsewhere
    # votes: cluster 0: 3 of 4, cluster 1: 2, cluster 2: 1, cluster 3: 1, cluster 4: 0
    for pct, want in ((75, [True, False, False, False, False]), (76, [False] * 5), (25, [True, True, True, True, False]),
                      (0, [True] * 5)):
        got = kmeans.vote(labels, sal, 5, 0.2, pct)
        assert got.dtype == torch.bool and got.tolist() == want, pct
        assert kr.vote(labels.numpy(), sal.numpy(), 5, 0.2, pct).tolist() == want, pct
    # exactly at the threshold is no vote (the mean must exceed it): cluster 1 of image 0 has mean 0.25
    assert kmeans.vote(labels[:1], sal[:1], 3, 0.25, 100).tolist() == [True, False, False]
    assert kmeans.vote(labels[:1], sal[:1], 3, 0.24, 100).tolist() == [True, True, False]
    with pytest.raises(ValueError, match="labels"):
        kmeans.vote(labels, sal[:, :3], 5)


def test_maximin_on_hand_made_arrays():
    from vdr import kmeans
    x = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 3.0], [1.0, 1.0], [-3.0, 0.0], [3.0, 0.0]])
    # largest norm: rows 1, 2, 4, 5 tie at 9 -> 1.  farthest from (3, 0): (-3, 0) at 36 -> 4.  then (0, 3) at 18 -> 2.  then rows 0
    # (9) and 3 (min(5, 17, 5) = 5) -> 0.  then 3.  Then every row is at distance 0 from the chosen set (row 5 duplicates row 1):
    # the tie goes to the lowest index, row 0 again -- a map with fewer than k distinct rows gets duplicate centres
    want = [1, 4, 2, 0, 3, 0]
    for k in range(1, 7):
        assert kr.maximin(x, k).tolist() == want[:k]
        assert kmeans.maximin(torch.from_numpy(x).unsqueeze(0), k)[0].tolist() == want[:k]
    two = torch.from_numpy(np.stack([x, x[::-1].copy()]))
    got = kmeans.maximin(two.to(torch.bfloat16), 3)
    assert got.tolist() == [[1, 4, 2], kr.maximin(x[::-1], 3).tolist()]
    rng = np.random.default_rng(0)
    r = rng.normal(size=(40, 32))
    assert kmeans.maximin(torch.from_numpy(r).unsqueeze(0), 7)[0].tolist() == kr.maximin(r, 7).tolist()


def _corr(t=6, gw=3, with_desc=True):
    import vdr
    nn12 = torch.tensor([[1, 0, 3, 2, 5, 4]], dtype=torch.int32)
    sim12 = torch.tensor([[0.5, 0.9, 0.9, 0.1, 0.7, 0.3]])
    sal1 = torch.tensor([[0.2, 0.4, 0.4, 0.9, 0.1, 1.0]])
    sal2 = torch.tensor([[0.5, 1.0, 0.5, 1.0, 1.0, 0.5]])
    mask = torch.tensor([[True, True, True, True, False, True]])
    c = vdr.Correspondences(nn12, sim12, nn12.clone(), sim12.clone(), sal1, sal2, mask, (2, gw), 4, 8)  # positionally, as before
    if with_desc:
        g = torch.Generator().manual_seed(0)
        c.desc1, c.desc2 = torch.randn(1, t, 32, generator=g).to(torch.bfloat16), torch.randn(1, t, 32, generator=g).to(torch.bfloat16)
    return c


def test_points_by_similarity_and_positional_construction_are_unchanged():
    c = _corr(with_desc=False)
    assert c.desc1 is None and c.desc2 is None
    p1, p2 = c.points(0)
    # masked positions 0, 1, 2, 3, 5 by descending sim12, ties by position: 1, 2, 0, 5, 3
    order = torch.tensor([1, 2, 0, 5, 3])
    want1 = torch.stack((order // 3, order % 3), 1).float() * 4 + 4.0
    buddy = torch.tensor([0, 3, 1, 4, 2])
    want2 = torch.stack((buddy // 3, buddy % 3), 1).float() * 4 + 4.0
    assert torch.equal(p1, want1) and torch.equal(p2, want2)
    q1, q2 = c.points(0, 2)
    assert torch.equal(q1, want1[:2]) and torch.equal(q2, want2[:2])
    r1, r2 = c.points(0, num_pairs=2, select="similarity")
    assert torch.equal(r1, q1) and torch.equal(r2, q2)
    with pytest.raises(ValueError, match="select"):
        c.points(0, 2, select="saliency")
    with pytest.raises(ValueError, match="keep_descriptors"):
        c.points(0, 2, select="kmeans")
    with pytest.raises(ValueError, match="num_pairs"):
        _corr().points(0, select="kmeans")
    with pytest.raises(ValueError, match="num_pairs"):
        _corr().points(0, 0, select="kmeans")


def test_points_by_kmeans_selection_with_a_stubbed_fit(monkeypatch):
    from vdr import kmeans
    from vdr.model import select_by_cluster
    c = _corr()
    seen = {}

    def fake_fit(x, k, init="maximin", **kw):
        seen.update(shape=tuple(x.shape), dtype=x.dtype, k=k, init=init)
        # the five buddies (positions 0, 1, 2, 3, 5): clusters 0, 0, 1, 1, 1 -- cluster 2 stays empty
        return kmeans.KMeans(torch.tensor([[0, 0, 1, 1, 1]], dtype=torch.int32), None, None, None, None, None)

    monkeypatch.setattr(kmeans, "fit", fake_fit)
    p1, p2 = c.points(0, num_pairs=3, select="kmeans")
    assert seen == dict(shape=(5, 64), dtype=torch.bfloat16, k=3, init="maximin")
    # rank = saliency1 * saliency2[nn12]: positions 0: .2 * 1 = .2, 1: .4 * .5 = .2, 2: .4 * 1 = .4, 3: .9 * .5 = .45, 5: 1 * 1 = 1
    # cluster 0 = {0, 1}: a tie at .2 -> position 0; cluster 1 = {2, 3, 5} -> 5; descending rank: 5, 0
    chosen = torch.tensor([5, 0])
    want1 = torch.stack((chosen // 3, chosen % 3), 1).float() * 4 + 4.0
    buddy = torch.tensor([4, 1])
    want2 = torch.stack((buddy // 3, buddy % 3), 1).float() * 4 + 4.0
    assert torch.equal(p1, want1) and torch.equal(p2, want2)
    seen.clear()
    c.points(0, num_pairs=50, select="kmeans")
    assert seen["k"] == 5  # min(num_pairs, n_bb)
    # the descriptors handed to the fit: both halves unit rows (to bf16 rounding), image 1's patch then its buddy's
    idx, desc = c.buddy_descriptors(0)
    assert idx.tolist() == [0, 1, 2, 3, 5]
    n = desc.float().reshape(5, 2, 32).norm(dim=-1)
    assert torch.allclose(n, torch.ones_like(n), atol=2e-2)
    want = torch.nn.functional.normalize(c.desc2[0][c.nn12[0][idx].long()].float(), dim=-1).to(torch.bfloat16)
    assert torch.equal(desc[:, 32:], want)
    # the selection alone: ties in rank go to the lowest position, inside a cluster and in the final order
    sel = select_by_cluster(torch.tensor([2, 2, 0, 0, 3]), torch.tensor([0.5, 0.5, 0.5, 0.7, 0.5]), 4)
    assert sel.tolist() == [3, 0, 4]
    # no masked buddy at all: two empty point sets, the fit is never called
    c.mask[:] = False
    seen.clear()
    p1, p2 = c.points(0, num_pairs=3, select="kmeans")
    assert p1.shape == (0, 2) and p2.shape == (0, 2) and not seen


def test_fit_refusals_need_no_device():
    from vdr import kmeans
    x = torch.zeros(2, 10, 32)
    for bad in (0, -1, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            kmeans.fit(x, bad)
    with pytest.raises(ValueError, match="exceeds the 10 rows"):
        kmeans.fit(x, 11)
    with pytest.raises(ValueError, match="init"):
        kmeans.fit(x, 2, init="kmeans++")
    with pytest.raises(ValueError, match="n_init"):
        kmeans.fit(x, 2, n_init=0)
    with pytest.raises(ValueError, match="n_init"):
        kmeans.fit(x, 2, n_init=3)  # maximin is deterministic
    with pytest.raises(ValueError, match="n_init"):
        kmeans.fit(x, 2, init=torch.zeros(2, 2, 32), n_init=2)
    with pytest.raises(ValueError, match="max_iter"):
        kmeans.fit(x, 2, max_iter=0)
    with pytest.raises(ValueError, match="sync_every"):
        kmeans.fit(x, 2, sync_every=-1)
    with pytest.raises(ValueError, match="multiple of 32"):
        kmeans.fit(torch.zeros(2, 10, 48), 2)
    with pytest.raises(TypeError, match="tensor"):
        kmeans.fit(np.zeros((2, 10, 32)), 2)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        kmeans.fit(torch.zeros(2, 10, 32, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="k_max"):
        kmeans.elbow(x, k_max=0)
    assert issubclass(kmeans.ConvergenceWarning, UserWarning)
    import vdr
    assert vdr.KMeans is kmeans.KMeans and [f for f in kmeans.KMeans.__dataclass_fields__] == ["labels", "centroids", "inertia",
                                                                                                "counts", "iters", "converged"]


def test_cosegment_refusals_need_no_device():
    import vdr
    from vdr.engine import Engine
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["vit_tiny16_224"]
    m.model_name = "vit_tiny16_224"
    m.engine = Engine.__new__(Engine)
    m.engine.cfg = m.cfg
    a = torch.zeros(1, 3, 224, 224)
    with pytest.raises(ValueError, match="facet"):
        m.cosegment(a, facet="keys")
    with pytest.raises(ValueError, match="hierarchy"):
        m.cosegment(a, bin=True, hierarchy=4)
    with pytest.raises(ValueError, match="out of range"):
        m.cosegment(a, layer=12)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.cosegment(a[0])
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            m.cosegment(a, k=bad)
    with pytest.raises(ValueError, match="exceeds the 196 patches"):
        m.cosegment(a, k=197)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.cosegment(a)
    m.cfg = vdr.ARCHS["siglip_base16_224"]
    with pytest.raises(ValueError, match="CLS"):
        m.cosegment(a)
    assert [f for f in vdr.Cosegmentation.__dataclass_fields__] == ["labels", "salient", "masks", "saliency", "kmeans"]
