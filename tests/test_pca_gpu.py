"""GPU: vdr_op_col_mean / vdr_op_covariance / vdr_op_pca_project (csrc/pca.hip) at op level against the float64 restatement
of their definitions (tests/pca_ref.py).

Designed inputs (integers in [-4, 4], columns of four different distributions, an integer `mean` vector) make every
centred value, product and partial sum exact in fp32, so all three ops must come back bit for bit whatever the summation
order.  Rows R: 2, 15, 16, 17 (one MFMA k-step and its neighbours), 1023, 1024, 1025 (the chunk boundary), 2049 (three
chunks); 16 rows are also one wave's share of a projection workgroup.  d: 32, 96, 160 (a ragged second column tile), 288
(three tiles: the off-diagonal pair (0, 2)).  Problems: 1 and 3.  The projection runs the same rows and widths with k = 1, 3,
8.  Wide maps: d = 2048 (16 column tiles, 136 pairs; with k = 8 the projection's components and mean take 72 KB of LDS, above
the 64 KB a kernel gets without opting in) and d = 1952 (a ragged sixteenth tile), exact as well.
Then: centring before the bf16 rounding (x = 1000 + q / 4), layout and batch independence (bitwise), the scaling, and
random inputs held to the entry-wise fp32 bounds."""
import pytest
import torch

import pca_ref as pref
from fixtures import ops  # noqa: F401
from ops_checks import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = (2, 15, 16, 17, 1023, 1024, 1025, 2049)
DIMS = (32, 96, 160, 288)
PROBLEMS = 3


_CACHE = {}


def _designed(R, d):
    """(x fp32 [3, R, d], integer mean [3, d]) -- made once per shape, shared, never written"""
    key = (R, d)
    if key not in _CACHE:
        _CACHE[key] = pref.designed(PROBLEMS, R, d, seed=100 * R + d)
    return _CACHE[key]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("R", ROWS)
def test_designed_covariance_is_exact_and_symmetric(ops, R, d):
    x, mean = _designed(R, d)
    want = torch.stack([pref.exact_f32_div(pref.gram(x[p], mean[p]), R - 1) for p in range(PROBLEMS)])
    for dtype in (torch.bfloat16, torch.float32):
        xd = x.to(dtype).cuda()
        m, cov = ops.covariance(xd, mean.cuda())
        assert_same_bits(m, mean, "mean is passed through")
        assert_same_bits(cov, want, ("cov", R, d, dtype))
        assert_same_bits(cov, cov.transpose(1, 2).contiguous(), "symmetry")
        _, solo = ops.covariance(xd[1:2], mean[1:2].cuda())
        assert_same_bits(solo, want[1:2], ("one problem", R, d, dtype))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("R", ROWS)
def test_designed_col_mean_is_exact(ops, R, d):
    x, _ = _designed(R, d)
    want = torch.stack([pref.exact_f32_div(x[p].double().sum(0), R) for p in range(PROBLEMS)])
    for dtype in (torch.bfloat16, torch.float32):
        xd = x.to(dtype).cuda()
        assert_same_bits(ops.col_mean(xd), want, ("mean", R, d, dtype))
        assert_same_bits(ops.col_mean(xd[2:3]), want[2:3], ("one problem", R, d, dtype))


@pytest.mark.parametrize("k", (1, 3, 8))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("R", ROWS)
def test_designed_projection_is_exact(ops, R, d, k):
    x, mean = _designed(R, d)
    comps = pref.designed_components(PROBLEMS, k, d, seed=R + d + k)
    want = torch.stack([pref.project(x[p], mean[p], comps[p])[0] for p in range(PROBLEMS)])
    assert bool((want == want.float().double()).all())
    wmm = torch.stack([want.amin(dim=(1, 2)), want.amax(dim=(1, 2))], dim=1).float()
    for dtype in (torch.bfloat16, torch.float32):
        xd = x.to(dtype).cuda()
        proj, mm = ops.pca_project(xd, mean.cuda(), comps.cuda())
        assert_same_bits(proj, want.float(), ("proj", R, d, k, dtype))
        assert_same_bits(mm, wmm, "minmax")
        proj1, mm1 = ops.pca_project(xd[1:2], mean[1:2].cuda(), comps[1:2].cuda())
        assert_same_bits(proj1, want[1:2].float(), "one problem")
        assert_same_bits(mm1, wmm[1:2], "one problem's minmax")


@pytest.mark.parametrize("R,d", ((70, 2048), (1030, 1952)))
def test_wide_maps_are_exact(ops, R, d):
    """the widest maps the ops take: every tile pair of the covariance, and the projection's opt-in LDS size at k = 8"""
    x, mean = pref.designed(2, R, d, seed=R + d)
    comps = pref.designed_components(2, 8, d, seed=d)
    wcov = torch.stack([pref.exact_f32_div(pref.gram(x[p], mean[p]), R - 1) for p in range(2)])
    wmean = torch.stack([pref.exact_f32_div(x[p].double().sum(0), R) for p in range(2)])
    wproj = torch.stack([pref.project(x[p], mean[p], comps[p])[0] for p in range(2)])
    assert bool((wproj == wproj.float().double()).all())
    xd = x.to(torch.bfloat16).cuda()
    assert_same_bits(ops.col_mean(xd), wmean, ("mean", R, d))
    _, cov = ops.covariance(xd, mean.cuda())
    assert_same_bits(cov, wcov, ("cov", R, d))
    assert_same_bits(cov, cov.transpose(1, 2).contiguous(), "symmetry")
    proj, mm = ops.pca_project(xd, mean.cuda(), comps.cuda())
    assert_same_bits(proj, wproj.float(), ("proj", R, d))
    assert_same_bits(mm, torch.stack([wproj.amin(dim=(1, 2)), wproj.amax(dim=(1, 2))], dim=1).float(), "minmax")
    proj3, _ = ops.pca_project(x.cuda(), mean.cuda(), comps[:, :3].contiguous().cuda())
    assert_same_bits(proj3, wproj[:, :, :3].contiguous().float(), ("proj k = 3, fp32", R, d))


def test_centring_precedes_the_bf16_rounding(ops):
    """x = 1000 + q / 4 in fp32 is not a bf16 number, x - 1000 is: the covariance is exact only if the subtraction comes first"""
    R, d = 1030, 96
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-8, 9, (2, R, d), generator=g).float()
    x = 1000.0 + q / 4
    mean = torch.full((2, d), 1000.0)
    want = torch.stack([pref.exact_f32_div((q[p].double() / 4).t() @ (q[p].double() / 4), R - 1) for p in range(2)])
    _, cov = ops.covariance(x.cuda(), mean.cuda())
    assert_same_bits(cov, want, "centred covariance")
    assert float(want.diagonal(dim1=1, dim2=2).min()) > 1.0  # (a rounding of x to bf16 first would leave multiples of 8: all wrong)


def test_layout_and_batch_independence_are_bitwise(ops):
    R, d = 300, 160
    g = torch.Generator().manual_seed(11)
    wide = (torch.randn(3, R, 3 * d, generator=g) * 2 + 0.5).to(torch.bfloat16).cuda()
    view = wide[:, :, d:2 * d]  # the middle facet of a qkv-like buffer: ld = 3 d, read in place
    assert view.stride(1) == 3 * d and not view.is_contiguous()
    x = view.contiguous()
    mean, cov = ops.covariance(x)
    comps = torch.randn(3, 3, d, generator=g).cuda()
    proj, mm = ops.pca_project(x, mean, comps, scale=True)
    # a strided view == its contiguous copy
    mv, cv = ops.covariance(view)
    pv, mmv = ops.pca_project(view, mean, comps, scale=True)
    for a, b, what in ((mv, mean, "mean"), (cv, cov, "cov"), (pv, proj, "proj"), (mmv, mm, "minmax")):
        assert_same_bits(a, b, ("view", what))
    # a problem inside a batch == its own run; two runs agree
    for p in range(3):
        m1, c1 = ops.covariance(x[p:p + 1])
        p1, mm1 = ops.pca_project(x[p:p + 1], m1, comps[p:p + 1], scale=True)
        for a, b, what in ((m1, mean[p:p + 1], "mean"), (c1, cov[p:p + 1], "cov"), (p1, proj[p:p + 1], "proj"), (mm1, mm[p:p + 1], "mm")):
            assert_same_bits(a, b, ("solo", p, what))
    m2, c2 = ops.covariance(x)
    assert_same_bits(m2, mean, "rerun mean")
    assert_same_bits(c2, cov, "rerun cov")
    assert_same_bits(ops.pca_project(x, mean, comps, scale=True)[0], proj, "rerun proj")
    # joint over 3 strided images == the same rows concatenated
    cat = view.reshape(1, 3 * R, d).contiguous()
    mj, cj = ops.covariance(view, joint=True)
    mc, cc = ops.covariance(cat)
    assert_same_bits(mj, mc, "joint mean")
    assert_same_bits(cj, cc, "joint cov")
    assert_same_bits(ops.col_mean(view, joint=True), mc, "joint col_mean")
    pj, mmj = ops.pca_project(view, mj, comps[:1], scale=False)
    pc, mmc = ops.pca_project(cat, mc, comps[:1], scale=False)
    assert pj.shape == (1, 3 * R, 3)
    assert_same_bits(pj, pc, "joint proj")
    assert_same_bits(mmj, mmc, "joint minmax")


def test_scaling_is_one_subtraction_and_one_division(ops):
    R, d, k = 517, 96, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, R, d, generator=g).cuda()
    mean = ops.col_mean(x)
    comps = torch.randn(2, k, d, generator=g).cuda()
    raw, mm = ops.pca_project(x, mean, comps, scale=False)
    assert_same_bits(mm, torch.stack([raw.amin(dim=(1, 2)), raw.amax(dim=(1, 2))], dim=1), "minmax of the unscaled output")
    scaled, mm2 = ops.pca_project(x, mean, comps, scale=True)
    assert_same_bits(mm2, mm, "minmax is that of the unscaled projection")
    raw, mm = raw.cpu(), mm.cpu()  # (the host's fp32 subtraction and division are the IEEE ones)
    lo, hi = mm[:, 0].view(2, 1, 1), mm[:, 1].view(2, 1, 1)
    assert_same_bits(scaled, (raw - lo) / (hi - lo), "scaled")
    assert float(scaled.min()) == 0.0 and float(scaled.max()) == 1.0
    # a constant map: max == min, returned as it is
    const = torch.full((1, 40, 32), 2.5).cuda()
    cm = torch.full((1, 32), 0.5).cuda()
    cc = torch.ones(1, 2, 32).cuda()
    raw, mm = ops.pca_project(const, cm, cc, scale=False)
    sc, _ = ops.pca_project(const, cm, cc, scale=True)
    assert float(mm[0, 0]) == float(mm[0, 1]) == 64.0
    assert_same_bits(sc, raw, "constant map")


@pytest.mark.parametrize("R,d,dtype", ((300, 768, torch.bfloat16), (1100, 256, torch.float32)))
def test_random_inputs_stay_inside_the_fp32_bounds(ops, R, d, dtype):
    g = torch.Generator().manual_seed(R + d)
    x = (torch.randn(2, R, d, generator=g) * (1 + torch.arange(d) % 5) + torch.randn(d, generator=g) * 3).to(dtype)
    mean, cov = ops.covariance(x.cuda())
    comps = torch.nn.functional.normalize(torch.randn(2, 3, d, generator=g), dim=-1)
    proj, mm = ops.pca_project(x.cuda(), mean, comps.cuda())
    mean, cov, proj = mean.cpu(), cov.cpu(), proj.cpu()
    for p in range(2):
        wm, bm = pref.col_mean(x[p])
        err = (mean[p].double() - wm).abs()
        assert bool((err <= bm).all()), ("mean", float((err / bm).max()))
        wc, bc = pref.covariance(x[p], mean[p])  # (the op's own mean: the covariance is defined for any vector)
        err = (cov[p].double() - wc).abs()
        assert bool((err <= bc).all()), ("cov", float((err / bc).max()))
        wp, bp = pref.project(x[p], mean[p], comps[p])
        err = (proj[p].double() - wp).abs()
        assert bool((err <= bp).all()), ("proj", float((err / bp).max()))
    assert bool((cov == cov.transpose(1, 2)).all())
