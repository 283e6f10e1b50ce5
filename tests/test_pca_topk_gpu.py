"""GPU: vdr_op_gram / vdr_op_sym_topk / vdr_op_pca_back_project / vdr_op_col_mean_any (csrc/pca.hip, csrc/pca_topk.hip) at op
level against the float64 restatement of their definitions (tests/pca_topk_ref.py), and vdr.pca.fit(solver="subspace")
against the golden files of sklearn and of the reference's pca_colorize.

gram, back-projection: designed inputs (integers in [-4, 4], an integer mean) make every centred value, product and partial
sum exact in fp32, so the ops must come back bit for bit whatever the summation order.  t: 2, 15, 16, 17 (one MFMA tile
corner), 127, 128, 129 (the row-tile boundary), 300 (three tiles, a ragged last one, every tile pair).  d: 32, 96, and the
column-chunk boundary VDR_GRAM_CHUNK - 32, VDR_GRAM_CHUNK, VDR_GRAM_CHUNK + 32 (= 288, two chunks); one binned width,
13 056 x 196 (51 chunks; the sums stay below 2^24).
sym_topk: planted spectra A = Q diag(lambda) Q^T; the contract is the float64 residual of the returned pairs, the vector
accuracy is Davis-Kahan's residual / gap -- derived, not tuned."""
import warnings

import numpy as np
import pytest
import torch

import pca_ref as pref
import pca_topk_ref as tref
from fixtures import ops  # noqa: F401
from ops_checks import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = (2, 15, 16, 17, 127, 128, 129, 300)
DIMS = tuple(sorted({32, 96, 288, tref.GRAM_CHUNK - 32, tref.GRAM_CHUNK, tref.GRAM_CHUNK + 32}))
PROBLEMS = 3
U = pref.U


_CACHE = {}


def _designed(t, d):
    key = ("designed", t, d)
    if key not in _CACHE:
        _CACHE[key] = pref.designed(PROBLEMS, t, d, seed=100 * t + d)
    return _CACHE[key]


def _planted(n, ratio):
    """(A fp32, eigenvalues descending, eigenvectors in columns) of the fp32 matrix itself -- made once, shared, never written"""
    key = ("planted", n, ratio)
    if key not in _CACHE:
        a, _, _ = tref.planted(n, tref.geometric(n, ratio), seed=n)
        w, v = np.linalg.eigh(a.astype(np.float64))
        _CACHE[key] = (a, w[::-1].copy(), v[:, ::-1].copy())
    return _CACHE[key]


def _want_gram(x, mean):
    z = pref.centred_bf16(x, mean)
    return pref.exact_f32_div(z @ z.t(), x.shape[0] - 1)


# ---- gram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", ROWS)
def test_designed_gram_is_exact_and_symmetric(ops, t, d):
    x, mean = _designed(t, d)
    want = torch.stack([_want_gram(x[p], mean[p]) for p in range(PROBLEMS)])
    for dtype in (torch.bfloat16, torch.float32):
        xd = x.to(dtype).cuda()
        m, g = ops.gram(xd, mean.cuda())
        assert_same_bits(m, mean, "mean is passed through")
        assert_same_bits(g, want, ("gram", t, d, dtype))
        assert_same_bits(g, g.transpose(1, 2).contiguous(), "symmetry")
        _, solo = ops.gram(xd[1:2], mean[1:2].cuda())
        assert_same_bits(solo, want[1:2], ("one problem", t, d, dtype))


def test_designed_gram_and_mean_of_a_binned_width_are_exact(ops):
    t, d = 196, 13056
    x, mean = pref.designed(1, t, d, seed=7)
    xd = x.to(torch.bfloat16).cuda()
    _, g = ops.gram(xd, mean.cuda())
    assert_same_bits(g, _want_gram(x[0], mean[0]).unsqueeze(0), "gram 196 x 13056")
    assert_same_bits(g, g.transpose(1, 2).contiguous(), "symmetry")
    assert_same_bits(ops.col_mean_any(xd), pref.exact_f32_div(x[0].double().sum(0), t).unsqueeze(0), "mean at d = 13056")


def test_the_wide_mean_is_col_mean_bit_for_bit(ops):
    g = torch.Generator().manual_seed(2)
    for t, d in ((300, 160), (1030, 2048)):
        x = (torch.randn(3, t, d, generator=g) * 3 + 0.5).to(torch.bfloat16).cuda()
        assert_same_bits(ops.col_mean_any(x), ops.col_mean(x), ("col_mean_any", t, d))
        assert_same_bits(ops.col_mean_any(x.float()), ops.col_mean(x.float()), ("col_mean_any fp32", t, d))


def test_gram_centring_precedes_the_bf16_rounding(ops):
    """x = 1000 + q / 4 in fp32 is not a bf16 number, x - 1000 is"""
    t, d = 130, 288
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-8, 9, (2, t, d), generator=g).float()
    x = 1000.0 + q / 4
    want = torch.stack([pref.exact_f32_div((q[p].double() / 4) @ (q[p].double() / 4).t(), t - 1) for p in range(2)])
    _, got = ops.gram(x.cuda(), torch.full((2, d), 1000.0).cuda())
    assert_same_bits(got, want, "centred gram")
    assert float(want.diagonal(dim1=1, dim2=2).min()) > 1.0


def test_gram_layout_and_batch_independence_are_bitwise(ops):
    t, d = 300, 288
    g = torch.Generator().manual_seed(11)
    wide = (torch.randn(3, t, 3 * d, generator=g) * 2 + 0.5).to(torch.bfloat16).cuda()
    view = wide[:, :, d:2 * d]  # ld = 3 d, read in place
    assert view.stride(1) == 3 * d and not view.is_contiguous()
    x = view.contiguous()
    mean, gram = ops.gram(x)
    assert_same_bits(mean, ops.col_mean(x), "gram's own mean is col_mean")
    mv, gv = ops.gram(view)
    assert_same_bits(mv, mean, "view mean")
    assert_same_bits(gv, gram, "view gram")
    for p in range(3):
        m1, g1 = ops.gram(x[p:p + 1])
        assert_same_bits(m1, mean[p:p + 1], ("solo mean", p))
        assert_same_bits(g1, gram[p:p + 1], ("solo gram", p))
    assert_same_bits(ops.gram(x)[1], gram, "rerun")
    assert bool((gram == gram.transpose(1, 2)).all())


@pytest.mark.parametrize("t,d,dtype", ((300, 768, torch.bfloat16), (129, 1056, torch.float32)))
def test_random_gram_stays_inside_the_fp32_bound(ops, t, d, dtype):
    g = torch.Generator().manual_seed(t + d)
    x = (torch.randn(2, t, d, generator=g) * (1 + torch.arange(d) % 5) + torch.randn(d, generator=g) * 3).to(dtype)
    mean, gram = ops.gram(x.cuda())
    mean, gram = mean.cpu(), gram.cpu()
    for p in range(2):
        want, bound = tref.gram(x[p], mean[p])
        err = (gram[p].double() - want).abs()
        assert bool((err <= bound).all()), ("gram", float((err / bound).max()))


# ---- back-projection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", ROWS + (1030,))  # the gram shapes (15 / 16 / 17: the sixteen row lanes), and two row chunks
def test_designed_back_projection_is_exact(ops, t, d):
    """integer weights: the raw sums are exact integers, so the only roundings are the float64 norm and the final division"""
    x, mean = (_designed(t, d) if t in ROWS else pref.designed(PROBLEMS, t, d, seed=t + d))
    for k in (1, 3, 8):
        gu = torch.Generator().manual_seed(t + d + k)
        u = torch.randint(-2, 3, (PROBLEMS, k, t), generator=gu).float()
        u[:, 0, 0] = 1.0  # (no all-zero first row)
        values = torch.ones(PROBLEMS, k)
        values[0, k - 1] = 0.0  # a dead component comes back as zeros
        raw = torch.stack([tref.back_project(x[p], mean[p], u[p], values[p])[1] for p in range(PROBLEMS)])
        assert bool((raw == raw.float().double()).all())
        norm = raw.pow(2).sum(2, keepdim=True).sqrt()  # float64; the squares are integers, their sum is exact in any order
        want = torch.where((values.unsqueeze(-1) > 0) & (norm > 0), raw / torch.where(norm > 0, norm, torch.ones_like(norm)),
                           torch.zeros_like(raw)).float()
        for dtype in (torch.bfloat16, torch.float32):
            got = ops.pca_back_project(x.to(dtype).cuda(), mean.cuda(), u.cuda(), values.cuda())
            assert_same_bits(got, want, ("back_project", t, d, k, dtype))
            length = got.cpu().double().norm(dim=2)
            assert bool(((length - 1).abs() <= 4 * U)[(values > 0) & (norm[..., 0] > 0)].all())
            assert float(got[0, k - 1].abs().max()) == 0.0
        solo = ops.pca_back_project(x[1:2].cuda(), mean[1:2].cuda(), u[1:2].cuda(), values[1:2].cuda())
        assert_same_bits(solo, want[1:2], ("one problem", t, d, k))


def test_back_projection_at_a_binned_width(ops):
    t, d, k = 196, 13056, 3
    x, mean = pref.designed(1, t, d, seed=9)
    u = torch.randint(-2, 3, (1, k, t), generator=torch.Generator().manual_seed(1)).float()
    raw = tref.back_project(x[0], mean[0], u[0], torch.ones(k))[1]
    got = ops.pca_back_project(x.to(torch.bfloat16).cuda(), mean.cuda(), u.cuda(), torch.ones(1, k).cuda())
    assert_same_bits(got, (raw / raw.pow(2).sum(1, keepdim=True).sqrt()).float().unsqueeze(0), "back_project 196 x 13056")


# ---- sym_topk -------------------------------------------------------------------------------------------------------------
def _check_pairs(a, w, v, val, vec, resid, tol, k, what, angles=True):
    """the contract of vdr_op_sym_topk on one problem: float64 residuals, Davis-Kahan angles, unit length, order, sign"""
    n = a.shape[0]
    a64, val64, vec64 = a.astype(np.float64), val.astype(np.float64), vec.astype(np.float64)
    res = np.linalg.norm(a64 @ vec64.T - vec64.T * val64, axis=0)
    print(what, "resid reported", resid, "float64 residual / lambda_1", res.max() / w[0], "value error", np.abs(val64 - w[:k]).max() / w[0])
    assert resid <= tol
    # + the fp32 rounding of the returned pair: |A| |dv| + |d theta| <= 2 u lambda_1
    assert res.max() <= (tol + 2 * U) * w[0], (what, res / w[0])
    assert np.abs(val64 - w[:k]).max() <= (tol + U) * w[0]
    assert np.abs(np.linalg.norm(vec64, axis=1) - 1).max() <= 4 * U
    assert np.all(np.diff(val64) <= 0)
    for j in range(k):
        at = int(np.argmax(np.abs(vec[j])))
        assert vec[j, at] > 0, (what, j)
        if angles:
            gap = np.abs(np.delete(w, j) - val64[j]).min()
            sin = tref.sine(vec64[j], v[:, j])
            assert sin <= res[j] / gap + 4 * U * np.sqrt(n), (what, j, sin, res[j] / gap)


@pytest.mark.parametrize("ratio", (0.5, 0.9))
@pytest.mark.parametrize("n", (2, 15, 16, 17, 33, 200, 768))
def test_sym_topk_on_planted_spectra(ops, n, ratio):
    a, w, v = _planted(n, ratio)
    ad = torch.from_numpy(a).unsqueeze(0).cuda()
    for k in (1, 3, 8):
        if k > n:
            continue
        val, vec, iters, resid = ops.sym_topk(ad, k)
        assert val.shape == (1, k) and vec.shape == (1, k, n) and iters.dtype == torch.int32 and int(iters[0]) < ops.TOPK_MAX_ITER
        _check_pairs(a, w, v, val[0].cpu().numpy(), vec[0].cpu().numpy(), float(resid[0]), ops.TOPK_TOL, k, (n, ratio, k, int(iters[0])))


def test_sym_topk_at_the_largest_size(ops):
    """n = 4096 (16 row blocks x 32 slabs): the residual contract and the eigenvalues against the planted ones -- Weyl:
    rounding A to fp32 moves an eigenvalue by at most ||E||_F <= u ||A||_F"""
    n, k = 4096, 3
    key = ("planted", n)
    if key not in _CACHE:
        _CACHE[key] = tref.planted(n, tref.geometric(n, 0.5), seed=n)
    a, q, lam = _CACHE[key]
    val, vec, iters, resid = ops.sym_topk(torch.from_numpy(a).unsqueeze(0).cuda(), k)
    val, vec = val[0].cpu().numpy().astype(np.float64), vec[0].cpu().numpy().astype(np.float64)
    res = np.linalg.norm(a.astype(np.float64) @ vec.T - vec.T * val, axis=0)
    print("n = 4096: iters", int(iters[0]), "resid", float(resid[0]), "float64 residual", res.max())
    assert float(resid[0]) <= ops.TOPK_TOL and res.max() <= (ops.TOPK_TOL + 2 * U) * lam[0]
    weyl = U * np.linalg.norm(lam)
    assert np.abs(val - lam[:k]).max() <= ops.TOPK_TOL * lam[0] + weyl + U * lam[0]
    for j in range(k):  # Davis-Kahan against the planted vectors: the fp32 rounding of A adds ||E|| / gap
        gap = np.abs(np.delete(lam, j) - val[j]).min() - weyl
        assert tref.sine(vec[j], q[:, j]) <= (res[j] + weyl) / gap + 4 * U * np.sqrt(n)


def test_sym_topk_near_degenerate_pair_returns_the_invariant_subspace(ops):
    n, k = 200, 4
    lam = tref.geometric(n, 0.5)
    lam[1] = lam[2] * (1 + 1e-3)
    a, _, _ = tref.planted(n, lam, seed=3)
    w, v = np.linalg.eigh(a.astype(np.float64))
    w, v = w[::-1], v[:, ::-1]
    val, vec, iters, resid = ops.sym_topk(torch.from_numpy(a).unsqueeze(0).cuda(), k)
    val, vec = val[0].cpu().numpy(), vec[0].cpu().numpy()
    _check_pairs(a, w, v, val, vec, float(resid[0]), ops.TOPK_TOL, k, ("near-degenerate", int(iters[0])), angles=False)
    # the pair's plane: each returned vector of the pair lies in span(v_2, v_3) up to residual / (gap to the REST of the spectrum)
    x = vec[1:3].astype(np.float64)
    res = np.linalg.norm(a.astype(np.float64) @ x.T - x.T * val[1:3].astype(np.float64), axis=0)
    for j in range(2):
        gap = min(abs(w[0] - val[1 + j]), abs(w[3] - val[1 + j]))
        out = x[j] - v[:, 1:3] @ (v[:, 1:3].T @ x[j])
        assert np.linalg.norm(out) <= res[j] / gap + 4 * U * np.sqrt(n), (j, np.linalg.norm(out), res[j] / gap)
    assert abs(x[0] @ x[1]) <= 8 * U * np.sqrt(n)  # and they span it
    for j in (0, 3):
        assert tref.sine(vec[j], v[:, j]) <= np.linalg.norm(a.astype(np.float64) @ vec[j] - val[j] * vec[j].astype(np.float64)) / \
            np.abs(np.delete(w, j) - val[j]).min() + 4 * U * np.sqrt(n)


def test_sym_topk_reports_no_convergence_and_fit_falls_back(ops):
    """a flat tail inside the block: lambda_3 .. lambda_17 at ratio 0.9999 cannot separate in max_iter iterations"""
    import vdr
    n, k = 64, 3
    lam = np.concatenate([[1.0, 0.5], 0.25 * 0.9999 ** np.arange(n - 2)])
    a, _, _ = tref.planted(n, lam, seed=6)
    ad = torch.from_numpy(a).unsqueeze(0).cuda()
    val, vec, iters, resid = ops.sym_topk(ad, k)
    print("flat tail: iters", int(iters[0]), "resid", float(resid[0]))
    assert int(iters[0]) == ops.TOPK_MAX_ITER and float(resid[0]) > ops.TOPK_TOL
    # the two separated pairs are still right, and the third is reported, not hidden
    assert np.abs(val[0, :2].cpu().numpy() - lam[:2]).max() <= 1e-5
    # fit on maps whose covariance has that spectrum (x = sqrt(t - 1) U diag(sqrt(lambda)) B^T, U orthonormal and centred):
    # one warning naming the count, and the eigh route's answer
    g = torch.Generator().manual_seed(4)
    t, d = 200, n
    xs = []
    for _ in range(2):
        r = torch.randn(t, d, generator=g, dtype=torch.float64)
        u = torch.linalg.qr(r - r.mean(0))[0]
        basis = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))[0]
        xs.append(np.sqrt(t - 1) * (u * torch.from_numpy(np.sqrt(lam))) @ basis.t())
    x = torch.stack(xs).float().cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        sub = vdr.pca.fit(x, k, solver="subspace")
    ours = [r for r in rec if issubclass(r.category, vdr.pca.ConvergenceWarning)]
    ref = vdr.pca.fit(x, k)
    print("fit on a flat tail: side", sub.side, "resid", sub.resid.tolist(), "warnings", [str(r.message) for r in ours])
    assert sub.side == "covariance" and bool((sub.resid > ops.TOPK_TOL).all())
    assert len(ours) == 1 and "2 of 2" in str(ours[0].message)
    assert torch.allclose(sub.components[:, :2], ref.components[:, :2], atol=1e-6)  # (same matrix, same solver, same batch)
    assert torch.allclose(sub.components, ref.components, atol=1e-5)
    assert torch.allclose(sub.explained_variance, ref.explained_variance, rtol=1e-12)


def test_sym_topk_is_bitwise_reproducible_and_batch_independent(ops):
    mats = [torch.from_numpy(_planted(200, r)[0]) for r in (0.5, 0.9)] + [torch.from_numpy(tref.planted(200, tref.geometric(200, 0.7), 1)[0])]
    batch = torch.stack(mats).cuda()
    whole = ops.sym_topk(batch, 3)
    again = ops.sym_topk(batch, 3)
    for a, b, what in zip(whole, again, ("values", "vectors", "iters", "resid")):
        assert_same_bits(a, b, ("rerun", what), dtype=a.dtype)  # (iters is int32)
    for p in (0, 2):  # alone == first of 3 == last of 3 (rolled so that it is)
        alone = ops.sym_topk(batch[p:p + 1], 3)
        rolled = ops.sym_topk(torch.roll(batch, 2 - p, 0).contiguous(), 3)
        for a, b, c, what in zip(alone, whole, rolled, ("values", "vectors", "iters", "resid")):
            assert_same_bits(a, b[p:p + 1], ("alone", p, what), dtype=a.dtype)
            assert_same_bits(a, c[2:3], ("moved to the end", p, what), dtype=a.dtype)
    assert len(set(whole[2].tolist())) > 1  # (the problems stop at different iterations: the done flags are per problem)


def test_sym_topk_on_a_rank_deficient_matrix(ops):
    n = 40
    lam = np.zeros(n)
    lam[:2] = (3.0, 1.0)
    a, q, _ = tref.planted(n, lam, seed=5)
    val, vec, iters, resid = ops.sym_topk(torch.from_numpy(a).unsqueeze(0).cuda(), 2)
    val, vec = val[0].cpu().numpy(), vec[0].cpu().numpy().astype(np.float64)
    print("rank 2: iters", int(iters[0]), "resid", float(resid[0]), val)
    assert float(resid[0]) <= ops.TOPK_TOL and int(iters[0]) <= 4
    assert np.abs(val - (3.0, 1.0)).max() <= 3 * (ops.TOPK_TOL + U)
    w = np.linalg.eigvalsh(a.astype(np.float64))[::-1]
    for j in range(2):
        res = np.linalg.norm(a.astype(np.float64) @ vec[j] - val[j] * vec[j])
        assert tref.sine(vec[j], q[:, j]) <= (res + U * 4) / np.abs(np.delete(w, j) - val[j]).min() + 4 * U * np.sqrt(n)


# ---- fit(solver="subspace") -----------------------------------------------------------------------------------------------
SIDES = {"pca_sk_64x64": "covariance", "pca_sk_196x768": "gram", "pca_sk_1024x256": "covariance"}


def _gates(p, g, x, what):
    comps = p.components[0].cpu().numpy()
    cos = 1 - pref.component_cosine(comps, g["components"])
    ev = np.abs(p.explained_variance[0].cpu().numpy() - g["explained_variance"]) / g["explained_variance"]
    evr = np.abs(p.explained_variance_ratio[0].cpu().numpy() - g["explained_variance_ratio"]) / g["explained_variance_ratio"]
    print(what, "side", p.side, "iters", p.iters.tolist(), "resid", p.resid.tolist(), "1-|cos|", cos.max(), "explained variance", ev.max(),
          "ratio", evr.max())
    assert np.all((comps * g["components"]).sum(-1) > 0)
    assert cos.max() <= pref.GATE_COS and ev.max() <= pref.GATE_EV and evr.max() <= pref.GATE_RATIO
    from vdr import ops
    assert float(p.resid[0]) <= ops.TOPK_TOL


@pytest.mark.parametrize("name", pref.SK_CASES)
def test_subspace_fit_against_sklearn(golden_dir, name):
    import vdr
    from vdr import ops
    g, x = pref.load_golden(golden_dir, name)
    xd = x.cuda()
    p = vdr.pca.fit(xd, 3, solver="subspace")
    assert p.side == SIDES[name] == vdr.pca.subspace_side(1, x.shape[0], x.shape[1], False)
    assert p.mean.shape == (1, x.shape[1]) and p.components.shape == (1, 3, x.shape[1]) and p.components.dtype == torch.float32
    _gates(p, g, x, name)
    rgb = vdr.pca.colorize(xd, (x.shape[0],), solver="subspace").cpu().numpy().astype(np.float64)
    err = np.abs(rgb - g["rgb_full"]).max()
    print(name, "rgb", err)
    assert err <= pref.GATE_RGB
    if p.side == "gram":
        # the scores are the projection on the same components, inside the projection's own fp32 bound plus what the bf16
        # centring of the Gram matrix (2^-9 per entry of z) may move a row's score: |z| . |c| * 2^-9
        assert p.scores.shape == (1, x.shape[0], 3)
        want, bound = pref.project(x, p.mean[0].cpu(), p.components[0].cpu())
        proj, _ = ops.pca_project(xd.unsqueeze(0), p.mean, p.components)
        assert bool(((proj[0].cpu().double() - want).abs() <= bound).all())
        # ... and what the solver's tolerance leaves of the eigenvector: sin <= resid / gap, gap >= 0.4 lambda_3 (the golden
        # maps have eigenvalue ratios <= 0.6), times the length sqrt(lambda_1 (t - 1)) of a column of scores
        z = (pref.f32(x) - p.mean[0].cpu()).double().abs()
        lam = p.explained_variance[0].cpu()
        assert np.all(g["eigen_ratios"] <= 0.6)
        slack = 2.0 ** -9 * (z @ p.components[0].cpu().double().abs().t()) + \
            float(ops.TOPK_TOL * lam[0] / (0.4 * lam[2]) * torch.sqrt(lam[0] * (x.shape[0] - 1)))
        err = (p.scores[0].cpu().double() - want).abs()
        print(name, "scores against the projection", float(err.max()), "allowed", float((bound + slack).min()))
        assert bool((err <= bound + slack).all())
    else:
        assert p.scores is None


def test_both_sides_agree_on_the_square_map(golden_dir):
    import vdr
    g, x = pref.load_golden(golden_dir, "pca_sk_64x64")
    xd = x.cuda()
    pc = vdr.pca.fit(xd, 3, solver="subspace", side="covariance")
    pg = vdr.pca.fit(xd, 3, solver="subspace", side="gram")
    assert (pc.side, pg.side) == ("covariance", "gram")
    _gates(pc, g, x, "64x64 covariance side")
    _gates(pg, g, x, "64x64 gram side")
    cos = 1 - pref.component_cosine(pc.components[0].cpu().numpy(), pg.components[0].cpu().numpy())
    ev = (pc.explained_variance - pg.explained_variance).abs() / pc.explained_variance
    print("sides: 1-|cos|", cos.max(), "explained variance", float(ev.max()))
    assert cos.max() <= pref.GATE_COS and float(ev.max()) <= pref.GATE_EV
    assert bool(((pc.components * pg.components).sum(-1) > 0).all())


def test_subspace_colorize_against_the_references_maps(golden_dir):
    import vdr
    g, x = pref.load_golden(golden_dir, "pca_ref_colorize")
    rgb = vdr.pca.colorize(x.numpy(), (32, 32), solver="subspace")
    bg = vdr.pca.colorize(x.numpy(), (32, 32), remove_bg=True, solver="subspace")
    assert isinstance(rgb, np.ndarray) and rgb.shape == (32, 32, 3) and rgb.dtype == np.float32
    e0, e1 = np.abs(rgb - g["rgb"]).max(), np.abs(bg - g["rgb_remove_bg"]).max()
    print("colorize(subspace)", e0, "remove_bg", e1)
    assert np.array_equal(bg[..., 0] > 0, g["mask"])
    assert e0 <= pref.GATE_REF_RGB and e1 <= pref.GATE_REF_RGB


def test_subspace_fit_does_not_depend_on_the_batch_it_came_in():
    """by construction, not by observation: every stage of the route is the library's own"""
    import vdr
    g = torch.Generator().manual_seed(8)
    for t, d in ((300, 768), (300, 256)):  # Gram side, covariance side
        x = (torch.randn(3, t, d, generator=g) * torch.linspace(4, 0.2, d) + torch.randn(d, generator=g)).to(torch.bfloat16).cuda()
        whole = vdr.pca.fit(x, 3, solver="subspace")
        for sl in (slice(0, 1), slice(2, 3), slice(1, 3)):
            part = vdr.pca.fit(x[sl], 3, solver="subspace")
            assert_same_bits(part.components, whole.components[sl], ("components", t, d, sl))
            assert torch.equal(part.explained_variance, whole.explained_variance[sl])
            if whole.scores is not None:
                assert_same_bits(part.scores, whole.scores[sl], ("scores", sl))


def test_a_wide_map_is_fitted_and_transform_says_where_it_stops():
    import vdr
    g = torch.Generator().manual_seed(12)
    t, d = 49, 4352  # 17 x 256: a binned tiny descriptor
    x = (torch.randn(2, t, 8, generator=g) @ torch.randn(8, d, generator=g) * 2 + torch.randn(2, t, d, generator=g) * 0.1).to(torch.bfloat16).cuda()
    p = vdr.pca.fit(x, 3, solver="subspace")
    assert p.side == "gram" and p.components.shape == (2, 3, d) and p.scores.shape == (2, t, 3)
    assert float((p.components.double().norm(dim=-1) - 1).abs().max()) <= 4 * U
    # against the float64 restatement of the same route on the host
    for b in range(2):
        _, comps, lam, _, scores = tref.fit(x[b].cpu(), 3, "gram", vdr.ops.TOPK_TOL, vdr.ops.TOPK_MAX_ITER)
        cos = 1 - pref.component_cosine(p.components[b].cpu().numpy(), comps.numpy())
        ev = (p.explained_variance[b].cpu() - lam).abs() / lam
        assert cos.max() <= pref.GATE_COS and float(ev.max()) <= pref.GATE_EV
    # beyond 2048 channels the colours are the fit's scores, min-max scaled: held here to an independent float64 projection
    # of the same map on the device's mean and components.  A score may differ from that projection by e = the bf16
    # centring of the Gram matrix (2^-9 |z| . |c|) + what the tolerance leaves of the eigenvector (sin <= tol lambda_1 / gap,
    # times the length sqrt(lambda_1 (t - 1)) of a column of scores) + the fp32 rounding of the score; (s - lo) / (hi - lo)
    # with every term off by at most e is off by at most 4 e / (range - 2 e).
    rgb = vdr.pca.colorize(x[0], (7, 7), solver="subspace").reshape(t, 3).cpu().double()
    want, _ = pref.project(x[0].cpu(), p.mean[0].cpu(), p.components[0].cpu())
    z = (pref.f32(x[0].cpu()) - p.mean[0].cpu()).double().abs()
    w = np.linalg.eigvalsh(tref.gram(x[0].cpu(), p.mean[0].cpu())[0].numpy())[::-1]
    gap = min(w[j] - w[j + 1] for j in range(3))
    e = float((2.0 ** -9 * (z @ p.components[0].cpu().double().abs().t())).max()) + \
        vdr.ops.TOPK_TOL * w[0] / gap * np.sqrt(w[0] * (t - 1)) + 2 * U * float(want.abs().max())
    rng = float(want.max() - want.min())
    err = float((rgb - (want - want.min()) / rng).abs().max())
    print("scores-coloured map against an independent projection", err, "allowed", 4 * e / (rng - 2 * e))
    assert err <= 4 * e / (rng - 2 * e) + 2 * U
    assert float(rgb.min()) == 0.0 and float(rgb.max()) == 1.0
    with pytest.raises(ValueError, match="stops at d = 2048"):
        p.transform(x)
    with pytest.raises(ValueError, match="at most 2048"):
        vdr.pca.fit(x, 3)  # the default route keeps its refusal
