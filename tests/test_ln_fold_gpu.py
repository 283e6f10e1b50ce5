"""GPU: the folded LayerNorm at op level, on designed inputs whose results are known exactly (oracle/ln_fold_designs.py).

  A  producer partials are bit-exact: every residual variant, LayerScale, the fp32 stream, ragged M, 1..24 groups
  B  the finalisers (ln_finalize_kernel, finalize_rows_if_last, the in-GEMM prologues) equal the float64 formula bit
     for bit, and each other; the counters are left zeroed
  C  the consumer is exact on designed rows with |mean| / sigma up to 192 and on constant rows
  D  padding rows and slots (NaN / Inf) do not leak; a NaN row changes only itself
  E  random data against float64 F.linear(F.layer_norm(x)) at ViT-B and DINOv2-g widths, plus the beta gate
"""
import math

import pytest
import torch

from fixtures import ops  # noqa: F401
from ops_checks import BF16_EPS, bf
from oracle import attn_designs as ad
from oracle import ln_fold_designs as lf

pytestmark = pytest.mark.gpu

EPS = lf.EPS


def _nan_part(G, stride):
    return torch.full((G, stride, 2), float("nan"), device="cuda")


def _partials_of(ops, x, variant=28, stride=None, fill=float("nan")):
    """partials of the bf16 rows x [M, D] through the producer itself: y = resid + (0 . 0^T + 0) = x"""
    M, D = x.shape
    stride = stride or M
    part = torch.full((D // 64, stride, 2), fill, device="cuda")
    z = torch.zeros((M, 64), dtype=torch.bfloat16, device="cuda")
    y = ops.linear_ln_stats(z, torch.zeros((D, 64), dtype=torch.bfloat16, device="cuda"), None, x, part, variant)
    assert torch.equal(y.view(torch.int16), x.view(torch.int16))  # (bitwise: NaN rows included)
    return part


def _run_producer(ops, case, variant, resid32=False, stats=False, stride=None):
    x, W, b, resid, gamma = case
    M, N = resid.shape
    stride = stride or M + 64
    part = _nan_part(N // 64, stride)
    kw = {}
    if resid32:
        kw = dict(resid32=resid.cuda().contiguous(), out32=torch.full((M, N), float("nan"), device="cuda"))
    if stats:
        kw["stats"] = torch.full((M, 2), float("nan"), device="cuda")
        kw["counters"] = torch.zeros((M + 63) // 64, dtype=torch.int32, device="cuda")
    y = ops.linear_ln_stats(bf(x).cuda(), bf(W).cuda(), b.cuda(), None if resid32 else bf(resid).cuda(), part, variant,
                            gamma=None if gamma is None else gamma.cuda(), eps=EPS, **kw)
    return y, part, kw


# ---- A ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 192, 768, 1024, 1088, 1536])
def test_producer_partials_bit_exact_every_variant(ops, N):
    M = 333
    for ls in (False, True):
        case = lf.integer_producer_case(M, N, 64, seed=N + ls, layerscale=ls)
        want_y = lf.model_producer(*case)
        want_p = lf.model_partials(want_y)
        for variant in range(22, 30):
            for r32 in (False, True):
                if r32 and variant == 25:
                    continue  # (the fp32 stream has no ring3k form: refused, tested in the ABI)
                y, part, kw = _run_producer(ops, case, variant, resid32=r32)
                what = f"N {N} variant {variant} layerscale {ls} resid32 {r32}"
                assert torch.equal(y.float().cpu(), want_y), what
                if r32:
                    assert torch.equal(kw["out32"].cpu(), want_y), what
                assert torch.equal(part[:, :M].cpu(), want_p), what
                assert torch.isnan(part[:, M:]).all(), f"{what}: wrote partial slots past M"


def test_producer_partials_persistent_and_of_the_stored_bf16_rows(ops):
    """ring4p (more tiles than the 512 workgroup slots) is bit-exact too; on random data the partials (of both residual
    epilogues) are those of the stored bf16 rows, not of the fp32 values before rounding"""
    M, N = 30011, 768
    case = lf.integer_producer_case(M, N, 64, seed=5, layerscale=True)
    want_y = lf.model_producer(*case)
    for variant in (26, 28):
        for r32 in (False, True):
            y, part, _ = _run_producer(ops, case, variant, resid32=r32)
            assert torch.equal(y.float().cpu(), want_y) and torch.equal(part[:, :M].cpu(), lf.model_partials(want_y)), (variant, r32)
    g = torch.Generator().manual_seed(6)
    M = 2000
    x = torch.randn(M, 256, generator=g)
    W = torch.randn(N, 256, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g) * 3
    for r32 in (False, True):
        y, part, _ = _run_producer(ops, (x, W, b, resid, None), 26, resid32=r32)
        lf.check_partials_of(part[:, :M], y.float().cpu(), f"random resid32 {r32}")


# ---- B ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 30011])
def test_finalisers_equal_the_float64_formula_bit_for_bit(ops, M):
    g = torch.Generator().manual_seed(M)
    for N in (768, 1088):
        x = torch.randn(M, 64, generator=g)
        W = torch.randn(N, 64, generator=g) * 0.2
        b = torch.randn(N, generator=g)
        resid = torch.randn(M, N, generator=g) * 2 + 40 * torch.randn(M, 1, generator=g)  # row means far from 0 too
        case = (x, W, b, resid, None)
        _, part, _ = _run_producer(ops, case, 28)
        want = lf.model_finalize(part[:, :M].cpu(), EPS)
        got = ops.ln_finalize(part, M, EPS)
        lf.check_stats_bitwise(got, want, f"ln_finalize M {M} N {N}")
        # three or more tile columns race per row block: 26 / 27 (256 wide: 3 at N = 768), 28 / 29 (128 wide: 6)
        for variant in (26, 27, 28, 29):
            for rep in range(2):  # the counters are left zeroed: a second launch finalises again
                _, p2, kw = _run_producer(ops, case, variant, stats=True)
                assert torch.equal(p2[:, :M], part[:, :M]), (variant, rep)
                lf.check_stats_bitwise(kw["stats"], want, f"finalize_rows_if_last M {M} N {N} variant {variant}")
                assert int(kw["counters"].abs().sum()) == 0, "counters not left zeroed"
    # the consumer fed the partials (finalised in the GEMM) is bitwise the consumer fed ln_finalize's statistics
    D = 768
    xr = bf(torch.randn(M, D, generator=g) + 3).cuda()
    part = _partials_of(ops, xr)
    st = ops.ln_finalize(part, M, EPS)
    Wf = bf(torch.randn(2304, D, generator=g) * 0.05).cuda()
    cs = Wf.float().sum(1)
    tb = torch.randn(2304, generator=g).cuda()
    for variant in (22, 23, 24, 26, 27, 28):
        a = ops.linear_ln_fold(xr, Wf, cs, tb, variant, stats=st, eps=EPS)
        c = ops.linear_ln_fold(xr, Wf, cs, tb, variant, part=part, eps=EPS)
        assert torch.equal(a, c), f"cpart != stats, variant {variant}"


# ---- C ----------------------------------------------------------------------------------------------------------
def _designed_consumer(ops, M, D, N, epi, variants, swiglu=False, seed=0, M_alloc=None):
    x = lf.cycled_rows(M, D, seed)
    W, b, gamma, beta = lf.designed_weights(N, D, seed + 1)
    Wf, cs, tb = ops.ln_fold_weights(W, b, gamma, beta, swiglu=swiglu)
    mf, mcs, mtb = lf.model_fold(W, b, gamma, beta, swiglu=swiglu)
    assert torch.equal(Wf.float(), mf) and torch.equal(cs, mcs) and torch.equal(tb, mtb)
    rows = M_alloc or M
    xa = torch.full((rows, D), float("nan"))
    xa[:M] = x
    xg = bf(xa).cuda()
    part = _partials_of(ops, xg[:M].contiguous(), stride=M + 64)
    st = torch.full((rows, 2), float("nan"), device="cuda")
    ops.ln_finalize(part, M, EPS, stats=st[:M])
    lf.check_stats_bitwise(st[:M], lf.model_finalize(lf.model_partials(x)), "designed statistics")
    return x, W, b, gamma, beta, Wf.cuda(), cs.cuda(), tb.cuda(), xg, part, st


@pytest.mark.parametrize("D", [768, 1536, 1088])
def test_consumer_fold_exact_on_designed_rows(ops, D):
    from vdr import EPI_BIAS
    M, N = 1000, 768
    x, W, b, gamma, beta, Wf, cs, tb, xg, part, st = _designed_consumer(ops, M, D, N, EPI_BIAS, None, seed=D)
    ref = lf.ref_fold(x, Wf.float().cpu(), W, b, beta)
    scale = lf.fold_noise_scale(x, Wf.float().cpu(), cs.cpu(), tb.cpu())
    excluded = {}
    for variant in range(22, 30):
        routes = [("stats", dict(stats=st))]
        if D <= 1024 and variant not in (25, 29):
            routes.append(("cpart", dict(part=part)))
        for name, kw in routes:
            y = ops.linear_ln_fold(xg, Wf, cs, tb, variant, M=M, eps=EPS, **kw)
            excluded[(variant, name)] = lf.check_exact_bf16(y, ref, f"D {D} variant {variant} {name}", scale=scale,
                                                            max_excluded_frac=0.1)
            const = (x.std(1) == 0).nonzero().flatten()
            assert torch.equal(y.float().cpu()[const], lf.bf16_round(tb.cpu()).expand(len(const), -1)), "constant rows"
    print(f"\n[ln-fold C] D {D}: elements within {lf.TIE_REL:.1e} x scale of a bf16 tie (excluded) of {M * N}: {excluded}")


def test_consumer_fold_exact_gelu_swiglu_and_8phase(ops):
    from vdr import EPI_BIAS, EPI_BIAS_GELU, EPI_SWIGLU
    M, D = 1000, 768
    # GELU at the existing GELU tolerance; SwiGLU: the x2 half of every gate pair reads its own colsum (n + 32)
    for epi, N, sw in ((EPI_BIAS_GELU, 3072, False), (EPI_SWIGLU, 2048, True)):
        x, W, b, gamma, beta, Wf, cs, tb, xg, part, st = _designed_consumer(ops, M, D, N, epi, None, swiglu=sw, seed=N)
        lin = lf.ref_fold(x, Wf.float().cpu(), W[lf.swiglu_perm(N)] if sw else W, b[lf.swiglu_perm(N)] if sw else b, beta)
        # (plus the epilogue's own fp32 noise, through the activation's slope: <= 1.1 for GELU, |x2| + |silu'| |x1| for SwiGLU)
        sc = lf.fold_noise_scale(x, Wf.float().cpu(), cs.cpu(), tb.cpu())
        if sw:
            v = lin.view(M, -1, 2, 32)
            s4 = sc.view(M, -1, 2, 32)
            band = (8 * 2.0 ** -24 * (s4[:, :, 0] * (v[:, :, 1].abs() + 1.1) + s4[:, :, 1] * v[:, :, 0].abs())).reshape(M, -1)
            ref = (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(M, -1)
        else:
            ref = torch.nn.functional.gelu(lin)
            band = 8 * 2.0 ** -24 * 1.1 * sc
        for variant in range(22, 30):
            routes = [dict(stats=st)] + ([dict(part=part)] if variant not in (25, 29) else [])
            for kw in routes:
                y = ops.linear_ln_fold(xg, Wf, cs, tb, variant, epilogue=epi, M=M, eps=EPS, **kw)
                lf.check_close(y, ref, BF16_EPS, 2e-3 + band, f"epi {epi} variant {variant} {list(kw)}")
    # variant 31 (the 8-phase kernel) at the shapes test_linear_8phase_variant_exact_and_bitwise uses, ragged M included
    # (x and the statistics readable, NaN, up to the next 256 rows)
    for M in (256 * 64, 256 * 64 - 100):
        x, W, b, gamma, beta, Wf, cs, tb, xg, part, st = _designed_consumer(ops, M, 256, 2048, EPI_BIAS, None, seed=M,
                                                                            M_alloc=256 * 64)
        ref = lf.ref_fold(x, Wf.float().cpu(), W, b, beta)
        y = ops.linear_ln_fold(xg, Wf, cs, tb, 31, stats=st, M=M, eps=EPS)
        n = lf.check_exact_bf16(y, ref, f"variant 31 M {M}", scale=lf.fold_noise_scale(x, Wf.float().cpu(), cs.cpu(), tb.cpu()),
                                max_excluded_frac=0.1)
        assert torch.equal(y, ops.linear_ln_fold(xg, Wf, cs, tb, 26, stats=st, M=M, eps=EPS)), "variant 31 != 26"
        print(f"\n[ln-fold C] variant 31 M {M}: {n} elements excluded of {y.numel()}")


# ---- D ----------------------------------------------------------------------------------------------------------
def test_padding_and_nan_rows_do_not_leak(ops):
    from vdr import EPI_BIAS
    M, D, N = 777, 768, 768
    x, W, b, gamma, beta, Wf, cs, tb, xg, part, st = _designed_consumer(ops, M, D, N, EPI_BIAS, None, seed=9, M_alloc=1024)
    ref = lf.ref_fold(x, Wf.float().cpu(), W, b, beta)
    scale = lf.fold_noise_scale(x, Wf.float().cpu(), cs.cpu(), tb.cpu())
    for fill in (float("nan"), float("inf")):
        part[:, M:] = fill
        st[M:] = fill
        xg[M:] = fill
        for variant in (22, 24, 26, 28, 29):
            for kw in ([dict(stats=st)] + ([dict(part=part)] if variant != 29 else [])):
                y = ops.linear_ln_fold(xg, Wf, cs, tb, variant, M=M, eps=EPS, **kw)
                lf.check_exact_bf16(y, ref, f"padding {fill} variant {variant}", scale=scale, max_excluded_frac=0.1)
    # a NaN in one valid row changes that row only
    base = ops.linear_ln_fold(xg, Wf, cs, tb, 26, stats=st, M=M, eps=EPS)
    xn = xg.clone()
    xn[5, 17] = float("nan")
    pn = _partials_of(ops, xn[:M].contiguous(), stride=M + 64)
    sn = ops.ln_finalize(pn, M, EPS)
    for kw in (dict(stats=sn), dict(part=pn)):
        y = ops.linear_ln_fold(xn, Wf, cs, tb, 26, M=M, eps=EPS, **kw)
        keep = torch.ones(M, dtype=torch.bool)
        keep[5] = False
        assert torch.equal(y[keep.cuda()], base[keep.cuda()]), "a NaN row leaked into other rows"
        assert torch.isnan(y[5].float()).all()


# ---- E ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,N,epi", [("vitb-qkv", 768, 2304, "bias"), ("vitb-fc1", 768, 3072, "gelu"),
                                          ("dinov2g-w12", 1536, 8192, "swiglu")])
def test_random_fold_against_float64(ops, name, D, N, epi):
    from vdr import EPI_BIAS, EPI_BIAS_GELU, EPI_SWIGLU
    E = {"bias": EPI_BIAS, "gelu": EPI_BIAS_GELU, "swiglu": EPI_SWIGLU}[epi]
    g = torch.Generator().manual_seed(D + N)
    M = 1000
    x = bf(torch.randn(M, D, generator=g) * 1.5 + 0.5 * torch.randn(M, 1, generator=g))
    W = torch.randn(N, D, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    sw = epi == "swiglu"
    Wf, cs, tb = ops.ln_fold_weights(W, b, gamma, beta, swiglu=sw)
    xg = x.cuda()
    part = _partials_of(ops, xg)
    st = ops.ln_finalize(part, M, EPS)
    # the fold's target for the weight it stores (float64, Wf = bf16(gamma W)) -- elementwise at test_linear_bias's
    # tolerance and the beta gate -- and F.linear(F.layer_norm(x)) with the unrounded weight: the beta gate
    lin = lf.ref_fold(x.float(), Wf.float(), W[lf.swiglu_perm(N)] if sw else W, b[lf.swiglu_perm(N)] if sw else b, beta)
    if sw:
        v = lin.view(M, -1, 2, 32)
        ref_f = (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(M, -1)
    else:
        ref_f = torch.nn.functional.gelu(lin) if epi == "gelu" else lin
    ref = lf.ref_consumer(x.float(), W, b, gamma, beta, EPS, epilogue=epi)
    betas = {}
    for variant in (22, 26, 28):
        for route, kw in (("stats", dict(stats=st)), ("cpart", dict(part=part))):
            if route == "cpart" and D > 1024:
                continue
            y = ops.linear_ln_fold(xg, Wf.cuda(), cs.cuda(), tb.cuda(), variant, epilogue=E, eps=EPS, **kw)
            lf.check_close(y, ref_f, BF16_EPS, 2e-3 * math.sqrt(D / 768), f"{name} variant {variant} {route}")
            yc = y.float().cpu()
            betas[(variant, route)] = (ad.check_unbiased(yc, ref_f.float(), f"{name} {variant} {route} (stored W)"),
                                       ad.check_unbiased(yc, ref.float(), f"{name} {variant} {route} (F.layer_norm)"))
    print(f"\n[ln-fold E] {name}: beta (stored W, F.layer_norm) "
          f"{', '.join(f'{k}: {v[0]:+.2e} {v[1]:+.2e}' for k, v in betas.items())}")
