"""CPU: the header and the binding of the guided-upsampling ops agree and the library exports them; every C-ABI refusal returns its
code before a device is touched, and so does every refusal of the Python layers (vdr.ops, vdr.upsample, the model method,
AnomalyMap, generate_features); vdr.upsample.nearest_patch against a brute-force arg-min of the distance to the patch centres, tie
rule included; the two restatements of tests/upsample_ref.py agree bit for bit on the all-ones design; an fp32 evaluation in another
summation order stays inside the restatement's bound and reaches a stated share of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import upsample_ref as ur
from fixtures import lib  # noqa: F401

PS = ((16, 16), (14, 14), (16, 8), (14, 7), (16, 4), (8, 8))
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -7


def _aligned(n=4096):
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) & ~15


def _args(ptr, **kw):
    a = dict(f=ptr, f_dtype=1, ld=64, image_stride=64 * 12, batch=2, gh=3, gw=4, C=64, guide=ptr, guide_dtype=0, Cg=3, H=32, W=40, p=16,
             s=8, radius=2, cs=0.5, cr=50.0, conf=None, y0=0, x0=0, y1=32, x1=40, work=ptr, out=ptr, out_dtype=1, stream=None)
    a.update(kw)
    return list(a.values())


def test_header_and_binding_agree(lib):
    from vdr import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdr.h")).read()
    for name, n in (("vdr_op_upsample_guided", 27), ("vdr_op_guide_lowres", 10)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        params = [q.strip() for q in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(params) == len(argtypes) == n, name
        for q, t in zip(params, argtypes):
            want = C.c_void_p if "*" in q else C.c_int64 if q.startswith("int64_t") else C.c_float if q.startswith("float") else C.c_int
            assert t is want, (name, q)
        assert hasattr(lib, name)
    assert re.search(r"size_t vdr_upsample_work_bytes\(int batch, int Cg, int gh, int gw\);", hdr)
    assert _lib.SYMBOLS["vdr_upsample_work_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert lib.vdr_abi_version() == 8  # only functions were added
    assert lib.vdr_upsample_work_bytes(2, 3, 5, 7) == 2 * 3 * 5 * 7 * 4 + 8  # rounded up to 16 bytes
    assert lib.vdr_upsample_work_bytes(0, 3, 5, 7) == 0


def test_op_refuses_bad_arguments_before_touching_a_device(lib):
    keep, p = _aligned()
    fn = lib.vdr_op_upsample_guided
    err = lambda: lib.vdr_last_error(None)  # noqa: E731
    for r in (0, 4, -1):
        assert fn(*_args(p, radius=r)) == UNSUPPORTED and b"radius" in err()
    for cg in (0, 5):
        assert fn(*_args(p, Cg=cg)) == UNSUPPORTED and b"1..4" in err()
    for name in ("f", "guide", "work", "out"):
        assert fn(*_args(p, **{name: None})) == INVALID and b"null" in err(), name
    for c in (0, 4, 60, -8):
        assert fn(*_args(p, C=c, ld=64)) == INVALID and b"multiple of 8" in err(), c
    assert fn(*_args(p, ld=56)) == INVALID and b"ld" in err()
    assert fn(*_args(p, image_stride=-8)) == INVALID
    for name in ("f", "work", "out"):
        assert fn(*_args(p, **{name: p + 8})) == INVALID and b"aligned" in err(), name
    assert fn(*_args(p, ld=68)) == INVALID and b"aligned" in err()
    assert fn(*_args(p, image_stride=64 * 12 + 4)) == INVALID and b"aligned" in err()
    assert fn(*_args(p, f_dtype=0, ld=66)) == INVALID and b"aligned" in err()  # fp32 rows: multiples of 4 elements
    assert fn(*_args(p, guide=p + 2)) == INVALID and fn(*_args(p, conf=p + 2)) == INVALID and b"aligned" in err()
    for kw in (dict(H=33), dict(W=41), dict(gh=4), dict(gw=3), dict(H=8), dict(p=16, s=16), dict(p=8, s=8)):
        assert fn(*_args(p, **kw)) == INVALID and b"patch + (g" in err(), kw
    for kw in (dict(s=3), dict(s=0), dict(p=0), dict(s=32)):
        assert fn(*_args(p, **kw)) == INVALID, kw
    assert fn(*_args(p, s=3)) == INVALID and b"divide" in err()
    for kw in (dict(y1=0), dict(x1=0), dict(y0=32), dict(y0=-1), dict(x0=-1), dict(y1=33), dict(x1=41), dict(y0=10, y1=10), dict(x0=9, x1=8)):
        assert fn(*_args(p, **kw)) == INVALID and b"box" in err(), kw
    for kw in (dict(cs=-1.0), dict(cr=-0.5), dict(cs=float("nan")), dict(cr=float("nan")), dict(cs=float("inf")), dict(cr=float("inf"))):
        assert fn(*_args(p, **kw)) == INVALID and b"finite" in err(), kw
    for kw in (dict(f_dtype=2), dict(out_dtype=3), dict(guide_dtype=2)):
        assert fn(*_args(p, **kw)) == INVALID and b"dtype" in err(), kw
    assert fn(*_args(p, batch=0)) == INVALID
    # a box of more than 2^31 - 1 pixels (the geometry alone is checked: nothing is dereferenced)
    side = 16 + 8 * 5999
    assert fn(*_args(p, H=side, W=side, gh=6000, gw=6000, y1=side, x1=side, batch=1, Cg=1)) == INVALID and b"2^31" in err()
    low = lib.vdr_op_guide_lowres
    assert low(None, 0, 1, 3, 32, 40, 16, 8, p, None) == INVALID and low(p, 0, 1, 3, 32, 40, 16, 8, None, None) == INVALID
    assert low(p, 0, 1, 5, 32, 40, 16, 8, p, None) == UNSUPPORTED and low(p, 0, 1, 3, 33, 40, 16, 8, p, None) == INVALID
    assert low(p, 0, 1, 3, 32, 40, 16, 5, p, None) == INVALID and low(p, 2, 1, 3, 32, 40, 16, 8, p, None) == INVALID


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_loud_failure_not_fallback(lib):
    from vdr import ops
    keep, p = _aligned()
    assert lib.vdr_op_upsample_guided(*_args(p)) == NO_DEVICE
    assert lib.vdr_op_upsample_guided(*_args(p, cs=0.0, cr=0.0, conf=p, y0=3, x0=5, y1=4, x1=6, f_dtype=0, out_dtype=0)) == NO_DEVICE
    assert lib.vdr_op_guide_lowres(p, 0, 1, 3, 32, 40, 16, 8, p, None) == NO_DEVICE
    with pytest.raises(TypeError, match="HIP device"):
        ops.upsample_guided(torch.zeros(1, 3, 4, 8), torch.zeros(1, 3, 32, 40), 16, 8)
    with pytest.raises(TypeError, match="HIP device"):
        ops.guide_lowres(torch.zeros(1, 3, 32, 40), 16, 8)


def test_python_refusals_need_no_device():
    import vdr
    from vdr import ops, pipeline, upsample
    from vdr.model import VitDescriptorModel
    f, g = torch.zeros(1, 3, 4, 8), torch.zeros(1, 3, 32, 40)
    with pytest.raises(TypeError):
        ops.upsample_guided(f[0], g, 16, 8)
    with pytest.raises(TypeError):
        ops.upsample_guided(f.half(), g, 16, 8)
    with pytest.raises(TypeError):
        ops.upsample_guided(f, g.double(), 16, 8)
    with pytest.raises(ValueError, match="divide"):
        ops.upsample_guided(f, g, 16, 5)
    with pytest.raises(ValueError, match="grid"):
        ops.upsample_guided(f, g, 16, 16)
    with pytest.raises(ValueError, match="grid"):
        ops.upsample_guided(torch.zeros(1, 3, 5, 8), g, 16, 8)
    with pytest.raises(ValueError, match="1..4"):
        ops.upsample_guided(f, torch.zeros(1, 5, 32, 40), 16, 8)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.upsample_guided(torch.zeros(1, 3, 4, 12), g, 16, 8)
    for r in (0, 4):
        with pytest.raises(ValueError, match="radius"):
            ops.upsample_guided(f, g, 16, 8, radius=r)
    for kw in (dict(sigma_spatial=0.0), dict(sigma_range=-1.0), dict(sigma_range=float("nan")), dict(sigma_range=1e-30)):
        with pytest.raises(ValueError, match="sigma"):
            ops.upsample_guided(f, g, 16, 8, **kw)
    for box in ((0, 0, 0, 5), (0, 0, 33, 40), (-1, 0, 4, 4), (5, 9, 5, 12), (0, 41, 3, 42)):
        with pytest.raises(ValueError, match="box"):
            ops.upsample_guided(f, g, 16, 8, box=box)
    with pytest.raises(ValueError, match="confidence"):
        ops.upsample_guided(f, g, 16, 8, confidence=torch.zeros(1, 3, 5))
    with pytest.raises(TypeError, match="out_dtype"):
        ops.upsample_guided(f, g, 16, 8, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="contiguous"):
        ops.upsample_guided(torch.zeros(1, 3, 8, 4).transpose(2, 3), g, 16, 8)
    assert ops.upsample_coefficients(8, float("inf"), float("inf")) == (0.0, 0.0)
    assert ops.upsample_coefficients(8, 1.0, 0.1) == (1.0 / 128.0, 1.0 / (2.0 * 0.1 * 0.1))
    with pytest.raises(ValueError, match="divide"):
        ops.guide_lowres(g, 16, 3)
    assert vdr.upsample is upsample
    with pytest.raises(TypeError):
        upsample.guided(torch.zeros(3, 4), g, 16, 8)
    with pytest.raises(ValueError, match="grid"):
        upsample.guided(torch.zeros(1, 3, 5), g, 16, 8)
    with pytest.raises(TypeError):
        upsample.guided_labels(torch.zeros(1, 3, 4), 2, g, 16, 8)
    with pytest.raises(ValueError, match="0 .. 1"):
        upsample.guided_labels(torch.full((1, 3, 4), 2), 2, g, 16, 8)
    with pytest.raises(ValueError):
        upsample.nearest_patch(33, 16, 8)
    amap = vdr.AnomalyMap(torch.zeros(1, 3, 4))
    with pytest.raises(ValueError, match="patch and stride"):
        amap.upsample_guided(g)
    with pytest.raises(ValueError, match="images"):
        amap.upsample_guided(torch.zeros(2, 3, 32, 40), patch=16, stride=8)
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["vit_tiny16_224"]
    m.model_name = "vit_tiny16_224"
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(ValueError, match="facet"):
        m.upsample_descriptors(x, facet="keys")
    with pytest.raises(ValueError, match="hierarchy"):
        m.upsample_descriptors(x, bin=True, hierarchy=4)
    with pytest.raises(ValueError, match="out of range"):
        m.upsample_descriptors(x, layer=12)
    with pytest.raises(ValueError, match="need a facet"):
        m.upsample_descriptors(x, facet=None, bin=True)
    with pytest.raises(ValueError, match="need a facet"):
        m.upsample_descriptors(x, facet=None, layer=0)
    with pytest.raises(ValueError, match="radius"):
        m.upsample_descriptors(x, radius=4)
    with pytest.raises(ValueError, match="sigma"):
        m.upsample_descriptors(x, sigma_range=0.0)
    with pytest.raises(ValueError, match="box"):
        m.upsample_descriptors(x, box=(0, 0, 225, 10))
    with pytest.raises(ValueError, match="out_dtype"):
        m.upsample_descriptors(x, out_dtype=torch.float16)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.upsample_descriptors(x[0])
    # generate_features: unknown keys are still refused, at both levels
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.generate_features(m, None, None, descriptor={"include_cls": True})
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.generate_features(m, None, None, descriptor={"facet": "key", "upsampling": {}})
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.generate_features(m, None, None, descriptor={"upsample": {"sigma": 1.0}})
    with pytest.raises(ValueError, match="radius"):
        pipeline.generate_features(m, None, None, descriptor={"upsample": {"radius": 5}})
    with pytest.raises(ValueError, match="sigma"):
        pipeline.generate_features(m, None, None, descriptor={"upsample": {"sigma_spatial": -1}})
    with pytest.raises(ValueError, match="facet"):
        pipeline.generate_features(m, None, None, descriptor={"facet": "nope", "upsample": {}})


@pytest.mark.parametrize("p,s", PS + ((16, 1), (6, 3), (10, 5)))
def test_nearest_patch_is_the_arg_min_of_the_distance_to_the_patch_centres(p, s):
    from vdr import upsample
    for n in (1, 2, 5, 9):
        size = p + (n - 1) * s
        got = upsample.nearest_patch(size, p, s)
        assert got.dtype == torch.int64 and got.tolist() == ur.nearest_patch(size, p, s, n).tolist()
        # twice the distance of pixel centre Y + 1/2 from patch centre s i + p / 2, in integers; on a tie the upper index
        Y = np.arange(size)[:, None]
        d2 = np.abs(2 * Y + 1 - 2 * s * np.arange(n)[None, :] - p)
        best = d2.min(axis=1, keepdims=True)
        upper = np.where(d2 == best, np.arange(n)[None, :], -1).max(axis=1)
        assert got.tolist() == upper.tolist()
        ties = (d2 == best).sum(axis=1) > 1
        assert ties.any() == (p % 2 == 0 and s % 2 == 1 and n > 1), (p, s, n)  # equal parity: no ties


@pytest.mark.parametrize("p,s,grid,r", ((16, 16, (5, 4), 1), (14, 7, (2, 3), 3), (16, 4, (9, 11), 2), (8, 8, (1, 1), 2), (16, 8, (5, 4), 3)))
def test_the_two_restatements_agree_on_the_all_ones_design(p, s, grid, r):
    gh, gw = grid
    H, W = p + (gh - 1) * s, p + (gw - 1) * s
    rng = np.random.default_rng(p + s + r)
    F = rng.integers(-8, 9, size=(2, gh, gw, 16)).astype(np.float32)
    G = rng.random((2, 3, H, W)).astype(np.float32)
    cs, cr = ur.coefficients(s, float("inf"), float("inf"))
    assert cs == 0 and cr == 0
    for box in (None, (1, 2, H - 1, W - 3)):
        a, info = ur.upsample_ref(F, G, p, s, r, cs, cr, box=box)
        b = ur.all_ones_ref(F, p, s, r, H, W, box=box)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(info["Z"], np.round(info["Z"])) and info["Z"].min() >= 1 and info["Z"].max() <= (2 * r + 1) ** 2


def _fp32_other_order(F, G, m, p, s, r, cs, cr):
    """the definition in plain float32, window positions in DESCENDING (a, b) order, expf by numpy's float32 exp, no hi / lo split,
    one accumulation per pixel"""
    F = np.asarray(F, dtype=np.float32)
    B, gh, gw, C = F.shape
    H, W = G.shape[2:]
    glr = ur.guide_lowres_ref(G, p, s)
    i0 = ur.nearest_patch(H, p, s, gh)[:, None]
    j0 = ur.nearest_patch(W, p, s, gw)[None, :]
    Y = np.arange(H)[:, None]
    X = np.arange(W)[None, :]
    out = np.zeros((B, H, W, C), dtype=np.float32)
    for b in range(B):
        acc = np.zeros((H, W, C), dtype=np.float32)
        Z = np.zeros((H, W), dtype=np.float32)
        for a in range(r, -r - 1, -1):
            for bb in range(r, -r - 1, -1):
                i, j = i0 + a + 0 * j0, j0 + bb + 0 * i0
                inside = (i >= 0) & (i < gh) & (j >= 0) & (j < gw)
                ic, jc = np.clip(i, 0, gh - 1), np.clip(j, 0, gw - 1)
                dy = ((2 * Y + 1 - p - 2 * s * i) / 2).astype(np.float32)
                dx = ((2 * X + 1 - p - 2 * s * j) / 2).astype(np.float32)
                dist2 = np.zeros((H, W), dtype=np.float32)
                for g in range(G.shape[1] - 1, -1, -1):
                    d = G[b, g] - glr[b, g][ic, jc]
                    dist2 = d * d + dist2
                t = -(dist2 * np.float32(cr) + (dx * dx + dy * dy) * np.float32(cs))
                w = np.where(inside & (t >= -64), np.exp(t) * m[b][ic, jc], np.float32(0)).astype(np.float32)
                acc = acc + w[:, :, None] * F[b][ic, jc]
                Z = Z + w
        out[b] = acc / Z[:, :, None]
    return out


def test_an_fp32_evaluation_in_another_order_stays_inside_the_bound():
    """worst error / bound over the entries: 0.254 with fp32 outputs (measured here; numpy's float32 exp, sums in descending window
    order, no split), so the bound is within a factor of four of what plain fp32 arithmetic reaches: neither vacuous nor
    loose by orders of magnitude.  The share asserted is a tenth of the bound."""
    p, s, r, gh, gw, C = 16, 8, 2, 5, 4, 24
    H, W = p + (gh - 1) * s, p + (gw - 1) * s
    rng = np.random.default_rng(3)
    F = ur.bf16_round(rng.standard_normal((2, gh, gw, C)) * 3 + 1)
    G = rng.random((2, 3, H, W)).astype(np.float32)
    m = (rng.random((2, gh, gw)) + 0.25).astype(np.float32)
    cs, cr = ur.coefficients(s, 0.8, 0.3)
    ref, info = ur.upsample_ref(F, G, p, s, r, cs, cr, conf=m, want_scale=True)
    assert info["tmax"] < 60 and (info["Z"] > 0).all()  # (no weight near the cut: the other order decides the same way)
    bnd = ur.bound(info["exact"], info["scale"], r, info["tmax"], False)
    got = _fp32_other_order(F, G, m, p, s, r, cs, cr)
    ratio = float((np.abs(got.astype(np.float64) - info["exact"]) / bnd).max())
    print(f"fp32 evaluation in another order: worst error / bound = {ratio:.3f}, |t|max {info['tmax']:.1f}")
    assert 0.1 <= ratio <= 1.0, ratio
