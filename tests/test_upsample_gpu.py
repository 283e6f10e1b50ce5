"""GPU: vdr_op_upsample_guided and vdr_op_guide_lowres (csrc/upsample.hip) at op level against the float64 restatement of the
definition (tests/upsample_ref.py).

Designed inputs, bit for bit (`_design`): features are integers in -8 .. 8; the guide is two-level, 1 where (X >= xe or X == 1)
xor (Y >= ye) with xe, ye on no patch border, the same in every guide channel; sigma_spatial = inf and sigma_range = 1e-3
(cr = 5e5).  A patch whose footprint lies on one side has g_lr 0 or 1; one that straddles a line has g_lr = k / p or a product
mix of such fractions, at least 1 / 16 away from both levels, so its exponent is below -5e5 / 256 = -1953 < -64 from BOTH
sides: every weight is exactly 0 or 1, Z is an integer count and any order of the sums is exact.  The column X == 1 is a
one-pixel line: its pixels find no patch of their level in reach (Z == 0, the fallback copy) wherever the window does not reach
across xe.  The second design adds confidences from {1 + 2^-10, 0.5, 0.25, 0} (w_hi = 1, w_lo = 2^-10 for the first): Z is a
multiple of 2^-10 below 2^6 and the numerators multiples of 2^-10 below 2^10, all exact in fp32, and the one division is
correctly rounded on both sides.  `_check_design` asserts in integers that the design has straddling patches, pixels with
Z == 0 and -- second design -- pixels whose numerator changes when w_lo is dropped.
Shapes: every (p, s) of PS on every grid of GRIDS; r, C, B, Cg and the three dtypes cycle through their values so that each
meets every (p, s) and every grid (C in 8, 32, 136, 264: ragged 128-channel tiles and more than two)."""
import numpy as np
import pytest
import torch

import upsample_ref as ur
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

PS = ((16, 16), (14, 14), (16, 8), (14, 7), (16, 4), (8, 8))
GRIDS = ((1, 1), (2, 3), (5, 4), (9, 11))
RS = (1, 2, 3)
CS = (8, 32, 136, 264)
DEV = "cuda"


def _cases():
    out = []
    for pi, (p, s) in enumerate(PS):
        for gi, grid in enumerate(GRIDS):
            k = pi * 4 + gi
            C = CS[(pi + gi) % 4]
            B = 1 if C * grid[0] * grid[1] > 20000 else (1, 3)[(k // 2) % 2]  # (the restatement of the widest map on the largest grid)
            out.append((p, s, grid, RS[k % 3], C, B, (1, 3)[(k // 3) % 2], bool(k % 2), bool((k // 2 + k) % 2),
                        bool((k // 4 + k) % 2)))
    return out


def _off_border(n, s):
    """a line position near n / 2 that is no multiple of s (and not 0)"""
    v = max(n // 2, 1)
    while v % s == 0 and s > 1:
        v += 1
    return v


def _design(p, s, grid, C, B, Cg, seed, conf=False):
    gh, gw = grid
    H, W = p + (gh - 1) * s, p + (gw - 1) * s
    rng = np.random.default_rng(seed)
    F = rng.integers(-8, 9, size=(B, gh, gw, C)).astype(np.float32)
    xe, ye = _off_border(W, s) + 1, _off_border(H, s)
    if xe % s == 0:
        xe += 1
    Y, X = np.mgrid[0:H, 0:W]
    G = (((X >= xe) | (X == 1)) ^ (Y >= ye)).astype(np.float32)
    G = np.broadcast_to(G, (B, Cg, H, W)).copy()
    for b in range(1, B):  # another picture per image
        G[b] = 1.0 - G[b] if b % 2 else G[b][:, ::-1, :]
    m = rng.choice(np.array([1 + 2.0 ** -10, 0.5, 0.25, 0.0], dtype=np.float32), size=(B, gh, gw)) if conf else None
    return F, G, m, H, W


def _run(ops, F, G, m, p, s, r, fbf, gbf, obf, sig=(float("inf"), 1e-3), box=None):
    f = torch.from_numpy(F).to(DEV).to(torch.bfloat16 if fbf else torch.float32)
    g = torch.from_numpy(G).to(DEV).to(torch.bfloat16 if gbf else torch.float32)
    c = None if m is None else torch.from_numpy(m).to(DEV)
    out = ops.upsample_guided(f, g, p, s, radius=r, sigma_spatial=sig[0], sigma_range=sig[1], confidence=c, box=box,
                              out_dtype=torch.bfloat16 if obf else torch.float32)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _expect_zero(p, s, grid, r):
    """shapes on which the design MUST have pixels with Z == 0: the 1 x 1 grid's only patch straddles, so every pixel falls back;
    the X == 1 line is out of reach of its own level when the window stops short of xe (r = 1 on the wide grids, s == p)"""
    return grid == (1, 1) or (r == 1 and grid[1] >= 4 and s == p)


def _check_design(F, G, m, p, s, r, info, expect_zero):
    glr = ur.guide_lowres_ref(G, p, s)
    assert ((glr > 0) & (glr < 1)).any(), "no straddling patch"
    frac = glr[(glr > 0) & (glr < 1)]
    assert (np.minimum(frac, 1 - frac) >= 1 / 16 - 1e-7).all()
    Z = info["Z"]
    assert np.array_equal(Z * 1024, np.round(Z * 1024)) and Z.max() < 64  # multiples of 2^-10 (integers without confidences)
    if m is None:
        assert np.array_equal(Z, np.round(Z))
    acc = info["acc"] * 1024
    assert np.array_equal(acc, np.round(acc)) and np.abs(acc).max() < 2 ** 24
    if expect_zero:
        assert (Z == 0).any(), "no pixel takes the fallback"


@pytest.mark.parametrize("p,s,grid,r,C,B,Cg,fbf,gbf,obf", _cases())
def test_designed_inputs_bit_for_bit(ops, p, s, grid, r, C, B, Cg, fbf, gbf, obf):
    F, G, _, H, W = _design(p, s, grid, C, B, Cg, seed=p * 100 + s + grid[0])
    cs, cr = ur.coefficients(s, float("inf"), 1e-3)
    ref, info = ur.upsample_ref(F, G, p, s, r, cs, cr, out_bf16=obf)
    _check_design(F, G, None, p, s, r, info, _expect_zero(p, s, grid, r))
    got = _run(ops, F, G, None, p, s, r, fbf, gbf, obf)
    assert got.shape == (B, H, W, C)
    assert _bits_equal(got, ref), f"{(got != ref).sum()} of {ref.size} entries differ, worst {np.abs(got - ref).max()}"


@pytest.mark.parametrize("p,s,grid,r,C,B,Cg,fbf,gbf,obf", _cases()[::2] + _cases()[1::6])
def test_designed_confidences_need_the_lo_operand(ops, p, s, grid, r, C, B, Cg, fbf, gbf, obf):
    F, G, m, H, W = _design(p, s, grid, C, B, Cg, seed=7 + p + s + grid[1], conf=True)
    cs, cr = ur.coefficients(s, float("inf"), 1e-3)
    ref, info = ur.upsample_ref(F, G, p, s, r, cs, cr, conf=m, out_bf16=False)
    _check_design(F, G, m, p, s, r, info, _expect_zero(p, s, grid, r))
    _, drop = ur.upsample_ref(F, G, p, s, r, cs, cr, conf=m, drop_lo=True)
    flagged = np.round(info["acc"] * 1024).astype(np.int64) != np.round(drop["acc"] * 1024).astype(np.int64)
    got = _run(ops, F, G, m, p, s, r, fbf, gbf, False)
    assert _bits_equal(got, ref), f"{(got != ref).sum()} of {ref.size} entries differ, worst {np.abs(got - ref).max()}"
    # (on the small grids, and wherever the footprints of overlapping patches all reach a line, every patch straddles: every weight
    # is 0 and every pixel falls back; the wide grids of non-overlapping patches must have live pixels)
    has_live = bool((info["Z"] != 0).any())
    assert has_live or not (s == p and grid[0] >= 5)
    if has_live:
        assert (m == np.float32(1 + 2.0 ** -10)).any() and flagged.any()
        live = flagged & (info["Z"] != 0)[..., None]
        ref_drop = (drop["acc"] / np.where(info["Z"] == 0, 1, info["Z"])[..., None]).astype(np.float32)
        changed = live & (ref_drop != ref)
        assert changed.any() and (got[changed] == ref[changed]).all() and (got[changed] != ref_drop[changed]).all()
    if obf:
        got16 = _run(ops, F, G, m, p, s, r, fbf, gbf, True)
        assert _bits_equal(got16, ur.bf16_round(ref))


# ---- one shared problem for views, boxes, batches and reruns ----------------------------------------------------
P0, S0, GRID0, R0, C0, B0, CG0 = 16, 8, (5, 4), 2, 136, 3, 3
_SHARED = {}


def _shared(ops):
    if not _SHARED:
        gh, gw = GRID0
        H, W = P0 + (gh - 1) * S0, P0 + (gw - 1) * S0
        rng = np.random.default_rng(11)
        F = ur.bf16_round(rng.standard_normal((B0, gh, gw, C0)))
        G = rng.random((B0, CG0, H, W)).astype(np.float32)
        m = rng.random((B0, gh, gw)).astype(np.float32)
        f = torch.from_numpy(F).to(DEV).to(torch.bfloat16)
        g = torch.from_numpy(G).to(DEV)
        c = torch.from_numpy(m).to(DEV)
        full = ops.upsample_guided(f, g, P0, S0, radius=R0, sigma_spatial=1.0, sigma_range=0.2, confidence=c)
        torch.cuda.synchronize()
        _SHARED.update(F=F, G=G, m=m, f=f, g=g, c=c, full=full, H=H, W=W)
    return _SHARED


def test_views_are_read_in_place_and_nothing_leaks(ops):
    sh = _shared(ops)
    gh, gw = GRID0
    t = gh * gw
    nan = float("nan")
    buf = torch.full((B0 + 2, t, 3 * C0), nan, dtype=torch.bfloat16, device=DEV)
    buf[1:B0 + 1, :, C0:2 * C0] = sh["f"].view(B0, t, C0)
    fv = buf[1:B0 + 1, :, C0:2 * C0].unflatten(1, (gh, gw))
    assert fv.data_ptr() != sh["f"].data_ptr() and fv.stride() == (t * 3 * C0, gw * 3 * C0, 3 * C0, 1)
    gbuf = torch.full((B0 + 2, CG0, sh["H"], sh["W"]), nan, device=DEV)
    gbuf[1:B0 + 1] = sh["g"]
    cbuf = torch.full((B0 + 2, gh, gw), nan, device=DEV)
    cbuf[1:B0 + 1] = sh["c"]
    n_out, guard = sh["full"].numel(), 64
    obuf = torch.full((n_out + 2 * guard,), nan, dtype=torch.bfloat16, device=DEV)
    n_work = B0 * CG0 * t
    n_work += -n_work % 4
    wbuf = torch.full((n_work + 2 * guard,), nan, device=DEV)
    out = ops.upsample_guided(fv, gbuf[1:B0 + 1], P0, S0, radius=R0, sigma_spatial=1.0, sigma_range=0.2, confidence=cbuf[1:B0 + 1],
                              out=obuf[guard:guard + n_out].view(sh["full"].shape), work=wbuf[guard:guard + n_work])
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr() + 2 * guard
    assert not torch.isnan(out.float()).any() and torch.equal(out, sh["full"])
    assert torch.isnan(obuf[:guard].float()).all() and torch.isnan(obuf[guard + n_out:].float()).all()
    assert torch.isnan(wbuf[:guard]).all() and torch.isnan(wbuf[guard + n_work:]).all()
    assert torch.equal(wbuf[guard:guard + B0 * CG0 * t].view(B0, CG0, gh, gw), ops.guide_lowres(sh["g"], P0, S0))
    # (the inputs are untouched)
    assert torch.isnan(buf[0].float()).all() and torch.isnan(buf[-1].float()).all() and torch.isnan(buf[:, :, :C0].float()).all()


def test_boxes_equal_the_region_of_the_full_output(ops):
    sh = _shared(ops)
    H, W = sh["H"], sh["W"]
    boxes = [(0, 0, H, W), (5, 7, 30, 22), (13, 9, 14, 10), (0, 0, 3, 5), (0, W - 5, 3, W), (H - 3, 0, H, 5), (H - 3, W - 5, H, W),
             (0, 0, 1, 1), (H - 1, W - 1, H, W)]
    for box in boxes:
        y0, x0, y1, x1 = box
        got = ops.upsample_guided(sh["f"], sh["g"], P0, S0, radius=R0, sigma_spatial=1.0, sigma_range=0.2, confidence=sh["c"], box=box)
        assert tuple(got.shape) == (B0, y1 - y0, x1 - x0, C0)
        assert torch.equal(got, sh["full"][:, y0:y1, x0:x1]), box


def test_an_image_does_not_depend_on_its_batch_and_runs_repeat(ops):
    sh = _shared(ops)
    again = ops.upsample_guided(sh["f"], sh["g"], P0, S0, radius=R0, sigma_spatial=1.0, sigma_range=0.2, confidence=sh["c"])
    assert torch.equal(again, sh["full"])
    for b in range(B0):
        solo = ops.upsample_guided(sh["f"][b:b + 1], sh["g"][b:b + 1], P0, S0, radius=R0, sigma_spatial=1.0, sigma_range=0.2,
                                   confidence=sh["c"][b:b + 1])
        assert torch.equal(solo[0], sh["full"][b]), b


RANDOM = [(16, 16, (5, 4), 1, 136, 2, 3, True, False, True), (14, 7, (9, 11), 3, 32, 1, 1, False, True, False),
          (16, 4, (5, 4), 2, 264, 1, 3, True, False, False), (8, 8, (2, 3), 3, 8, 3, 1, False, False, True),
          (16, 8, (9, 11), 2, 32, 1, 3, True, True, True), (14, 14, (1, 1), 1, 136, 3, 1, True, False, False)]


@pytest.mark.parametrize("p,s,grid,r,C,B,Cg,fbf,gbf,obf", RANDOM)
def test_random_inputs_stay_inside_the_bound(ops, p, s, grid, r, C, B, Cg, fbf, gbf, obf):
    gh, gw = grid
    H, W = p + (gh - 1) * s, p + (gw - 1) * s
    rng = np.random.default_rng(p + 3 * s + r)
    F = ur.bf16_round(rng.standard_normal((B, gh, gw, C)) * 3 + 1)
    G = rng.random((B, Cg, H, W)).astype(np.float32)
    if gbf:
        G = ur.bf16_round(G)
    m = rng.random((B, gh, gw)).astype(np.float32)
    sig = (0.8, 0.15)
    cs, cr = ur.coefficients(s, *sig)
    ref, info = ur.upsample_ref(F, G, p, s, r, cs, cr, conf=m, out_bf16=obf, want_scale=True)
    bnd = ur.bound(info["exact"], info["scale"], r, info["tmax"], obf)
    got = _run(ops, F, G, m, p, s, r, fbf, gbf, obf, sig=sig)
    err = np.abs(got.astype(np.float64) - info["exact"])
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    print(f"upsample_guided p {p} s {s} grid {grid} r {r} C {C} out {'bf16' if obf else 'fp32'}: worst error / bound = {ratio:.3f}, "
          f"|t|max {info['tmax']:.1f}")
    assert (err <= bnd).all(), ratio


@pytest.mark.parametrize("p,s", PS)
@pytest.mark.parametrize("gbf", (False, True))
def test_guide_lowres_bit_for_bit_on_integer_guides(ops, p, s, gbf):
    gh, gw = 5, 4
    H, W = p + (gh - 1) * s, p + (gw - 1) * s
    G = np.random.default_rng(p + s).integers(0, 256, size=(2, 3, H, W)).astype(np.float32)
    g = torch.from_numpy(G).to(DEV).to(torch.bfloat16 if gbf else torch.float32)
    got = ops.guide_lowres(g, p, s).cpu().numpy()
    assert got.shape == (2, 3, gh, gw) and _bits_equal(got, ur.guide_lowres_ref(G, p, s))


def test_all_ones_design_is_the_window_mean(ops):
    p, s, grid, r, C = 16, 8, (5, 4), 2, 32
    F, G, _, H, W = _design(p, s, grid, C, 2, 1, seed=5)
    got = _run(ops, F, G, None, p, s, r, True, False, False, sig=(float("inf"), float("inf")))
    assert _bits_equal(got, ur.all_ones_ref(F, p, s, r, H, W))
