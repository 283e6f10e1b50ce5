"""GPU, through the C ABI: the QuickGELU / tanh-GELU GEMM epilogues and the one-query attention pooling kernel.

Epilogues (vdr_op_linear, vdr_op_linear_packed, vdr_op_linear_ln_fold with VDR_EPI_BIAS_QUICK_GELU / _GELU_TANH):
  * inputs whose fp32 pre-activation is known exactly (clip_ref.epilogue_test_inputs), reference = float64 activation of
    it: EVERY element within 1 bf16 ulp of the correctly rounded value, and the share of elements that are not the
    correctly rounded value <= 1e-3.  The cap: the formula's fp32 error, a few ulp including v_exp_f32 / v_rcp_f32, is
    about 2^-21 relative against a bf16 ulp of 2^-8, so a flip needs the value within about 2^-13 of a rounding
    boundary -- 1 to 2.5e-4 of the elements; the cap leaves 4 x over that.  tests/test_clip_cpu.py shows the formula
    alone (exact exp2 and division) at <= 2.5e-4 on the same inputs.
  * the same launch on every tile family gives the same bits (ring3, ring4 packed, 8-phase; LayerNorm fold: 22 / 26 / 28 / 31).
Pooling (vdr_op_attention_pool): exact on designed inputs, an fp32 reference on random ones, bitwise batch invariance.
"""
import math

import pytest
import torch

import clip_ref as cr
from fixtures import ops  # noqa: F401
from ops_checks import BF16_EPS, bf

pytestmark = pytest.mark.gpu

KINDS = {"quick_gelu": "EPI_BIAS_QUICK_GELU", "gelu_tanh": "EPI_BIAS_GELU_TANH"}


def _epi(kind):
    import vdr
    return getattr(vdr, KINDS[kind])


# (M, N, K, variants): the first is a launch the 8-phase kernel takes (512 tiles of 256 x 256: two full rounds), the second
# the headline fc1 width on ring4 / ring3, the rest ragged in M and N
EPI_SHAPES = [(256 * 64, 2048, 256, (22, 26, 31)), (2048, 3072, 768, (22, 26, 27)), (333, 776, 320, (22, 24, 26, 28, 29)),
              (197 * 3 + 5, 1000, 128, (23, 25, 26, 28))]


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("M,N,K,variants", EPI_SHAPES)
def test_linear_activation_epilogue_one_ulp_and_flip_share(ops, kind, M, N, K, variants):
    x, W, b = cr.epilogue_test_inputs(M, N, K, seed=M + N + K)
    xd, Wd, bd = bf(x).cuda(), bf(W).cuda(), b.cuda()
    assert torch.equal(xd.float().cpu(), x) and torch.equal(Wd.float().cpu(), W)  # the grids are bf16-exact
    pre = cr.exact_preactivation(xd.float(), Wd.float(), bd)       # float64 on the device, exact
    exact = cr.exact_activation_fp64(pre, kind)
    first = None
    for v in variants:
        packed = v in (26, 27, 28, 29)
        y = ops.linear(xd, ops.pack_linear_weight(Wd) if packed else Wd, bd, epilogue=_epi(kind), variant=v, packed=packed)
        assert torch.isfinite(y.float()).all()
        dist = cr.bf16_ulp_distance(y, exact)
        share = (dist != 0).double().mean().item()
        print(f"{kind} {M}x{N}x{K} variant {v}: max bf16 ulp distance {int(dist.max())}, not correctly rounded {share:.3e} "
              f"({int((dist != 0).sum())} of {dist.numel()})")
        assert int(dist.max()) <= 1, (kind, v)
        assert share <= 1e-3, (kind, v, share)
        if first is None:
            first = y
        else:
            assert torch.equal(first, y), f"variant {v} differs bitwise from variant {variants[0]}"
    # the library's own choice (variant 0) gives the same bits
    assert torch.equal(first, ops.linear(xd, Wd, bd, epilogue=_epi(kind)))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_activation_tail_sweep_and_non_finite_inputs(ops, kind):
    """x = 0, W = 0: the pre-activation of column c is exactly the fp32 bias vals[c].  Sweep -12 .. 12 (the tails: large
    |x| gives x or -0), the extremes of the output format, and NaN / +-inf as csrc/vdr_dev.h states them."""
    K = 64
    fmax = torch.finfo(torch.bfloat16).max  # (the largest finite OUTPUT: fp32 values beyond it round to inf in any bf16 epilogue)
    vals = torch.cat([torch.linspace(-12, 12, 4096 - 16), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 65504.0, -65504.0, 1e20, -1e20,
                                                                         3e38, -3e38, fmax, -fmax, 1e-36, -1e-36, 30.0, -30.0])])
    N = vals.numel()
    y = ops.linear(bf(torch.zeros(4, K)).cuda(), bf(torch.zeros(N, K)).cuda(), vals.cuda(), epilogue=_epi(kind)).cpu()
    assert torch.isfinite(y.float()).all(), "finite x must give a finite result"
    exact = cr.exact_activation_fp64(vals, kind).expand(4, N)
    dist = cr.bf16_ulp_distance(y, exact)
    # (below |x| 2^-125 the formula's range ends: -0 for a true value of that size, see tests/test_clip_cpu.py)
    ok = (dist <= 1) | (exact.abs() <= vals.double().abs().expand(4, N) * 2.0 ** -125)
    assert ok.all(), (kind, vals[(~ok)[0]][:5])
    big = vals.abs() >= 1e20
    assert torch.equal(y[0][big & (vals > 0)].float(), bf(vals[big & (vals > 0)]).float())
    neg = y[0][big & (vals < 0)].float()
    assert (neg == 0).all() and torch.signbit(neg).all()
    sp = torch.tensor([float("nan"), float("inf"), float("-inf")] + [0.0] * 5)
    z = ops.linear(bf(torch.zeros(2, K)).cuda(), bf(torch.zeros(8, K)).cuda(), sp.cuda(), epilogue=_epi(kind)).float().cpu()[0]
    assert torch.isnan(z[0]) and z[1] == float("inf") and torch.isnan(z[2])  # NaN propagates; +inf -> +inf; -inf -> NaN (-inf * 0)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ln_fold_consumer_with_the_new_epilogues(ops, kind):
    """vdr_op_linear_ln_fold with the two activations: the ring3 / ring4 / 8-phase consumers give the same bits, and they are
    the activation of float64 F.linear(F.layer_norm(x)) to the tolerance the erf-GELU consumer is held to."""
    g = torch.Generator().manual_seed(17)
    M, D, N, eps = 256 * 64, 768, 3072, 1e-5   # 64 x 12 = 768 tiles, three full rounds: the 8-phase kernel takes it
    x = bf(torch.randn(M, D, generator=g) * 1.3 + 0.2).cuda()
    W = torch.randn(N, D, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    Wf, cs, tb = (t.cuda() for t in ops.ln_fold_weights(W, b, gamma, beta))
    part = torch.full((D // 64, M, 2), float("nan"), device="cuda")
    z = torch.zeros((M, 64), dtype=torch.bfloat16, device="cuda")
    ops.linear_ln_stats(z, torch.zeros((D, 64), dtype=torch.bfloat16, device="cuda"), None, x, part, 28)  # partials of x itself
    st = ops.ln_finalize(part, M, eps)
    outs = {v: ops.linear_ln_fold(x, Wf, cs, tb, v, epilogue=_epi(kind), stats=st, eps=eps) for v in (22, 26, 28, 31)}
    for v in (26, 28, 31):
        assert torch.equal(outs[22], outs[v]), f"fold consumer: variant {v} differs bitwise from 22"
    assert torch.equal(outs[22], ops.linear_ln_fold(x, Wf, cs, tb, 26, epilogue=_epi(kind), part=part, eps=eps)), "in-GEMM statistics"
    # float64 LN(x) W^T + b with the weight the device multiplies: rstd ((x - mean) Wf^T) + tbias, Wf = bf16(gamma W)
    xc = x.double() - x.double().mean(1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(1, keepdim=True) + eps)
    ref = cr.exact_activation_fp64(rstd * (xc @ Wf.double().t()) + tb.double(), kind)
    err = (outs[22].double() - ref).abs()
    bound = 2e-3 + BF16_EPS * ref.abs()  # (test_linear_gelu's tolerance: one bf16 rounding + the fold's fp32 noise)
    print(f"{kind} fold consumer: max err {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    # and the unfolded path (explicit LayerNorm, then vdr_op_linear) agrees with it to bf16 noise
    h = ops.layernorm(x, gamma.cuda(), beta.cuda(), eps)
    plain = ops.linear(h, bf(W).cuda(), b.cuda(), epilogue=_epi(kind))
    rel = ((plain.double() - outs[22].double()).norm() / outs[22].double().norm()).item()
    print(f"{kind}: folded vs explicit LayerNorm + linear: rel L2 {rel:.3e}")
    assert rel <= 8e-3


# ---- vdr_op_attention_pool ----------------------------------------------------------------------------------------------
HEAD_DIMS = [32, 64, 96, 128]
POOL_N = [1, 7, 196, 577, 1024, 4096]


def _pool_ref(q, kv, B, n, H, dh):
    """fp32 torch reference from the same bf16 k / v"""
    D = H * dh
    kvf = kv.float().reshape(B, n, -1)
    return cr.pool_attention(q.float(), kvf[..., :D], kvf[..., D:2 * D], H)


@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_pool_all_keys_equal_gives_the_mean_exactly(ops, dh):
    """Every key of an image equal -> every score equal -> every p = 2^0 = 1: out = bf16(sum_j v_j / n) exactly (small integer
    V: the sum is exact, the one IEEE division and the one bf16 rounding are the kernel's)."""
    g = torch.Generator().manual_seed(dh)
    H = 3
    D = H * dh
    for n in POOL_N:
        B = 2
        q = torch.randn(D, generator=g)
        k = bf(torch.randn(B, 1, D, generator=g)).expand(B, n, D)
        v = torch.randint(-8, 9, (B, n, D), generator=g).float()
        kv = torch.cat([bf(k), bf(v)], dim=-1).reshape(B * n, 2 * D).contiguous().cuda()
        out = ops.attention_pool(q.cuda(), kv, B, n, H, dh).cpu()
        want = bf(v.sum(1) / float(n))  # fp32 division of an exact integer sum, then one rounding
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), (dh, n)


@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_pool_one_dominant_key_gives_its_value_row_exactly(ops, dh):
    """One key per (image, head) ahead of all others by a score margin of >= 400 in the exponent of 2: every other 2^x
    underflows to 0 -> out = that key's V row, bit for bit.  The winner sits at a different position per image and head
    (first key, last key, a ragged tail position)."""
    g = torch.Generator().manual_seed(100 + dh)
    H, B = 2, 3
    D = H * dh
    for n in POOL_N:
        q = torch.zeros(H, dh)
        q[:, 0] = 16.0                                   # score = 16 k[0] / sqrt(dh): k[0] = 64 sqrt(dh)/4 ... below
        k = bf(torch.randn(B, n, H, dh, generator=g) * 0.5)
        k[..., 0] = 0.0
        v = bf(torch.randn(B, n, H, dh, generator=g) * 3)
        win = torch.zeros(B, H, dtype=torch.long)
        for b in range(B):
            for h in range(H):
                win[b, h] = (0, n - 1, (7 * b + 3 * h + n // 2) % n)[(b + h) % 3]
                k[b, win[b, h], h, 0] = 32.0 * math.ceil(math.sqrt(dh))  # margin: 16 * 32 sqrt(dh) / sqrt(dh) * log2(e) > 700
        kv = torch.cat([k.reshape(B, n, D), v.reshape(B, n, D)], dim=-1).reshape(B * n, 2 * D).contiguous().cuda()
        out = ops.attention_pool(q.reshape(D).cuda(), kv, B, n, H, dh).cpu().reshape(B, H, dh)
        for b in range(B):
            for h in range(H):
                assert torch.equal(out[b, h].view(torch.int16), v[b, win[b, h], h].view(torch.int16)), (dh, n, b, h)


@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_pool_random_against_fp32_reference_and_batch_invariance(ops, dh):
    """Random inputs against the fp32 torch reference computed from the same bf16 k / v (tolerance of the attention op
    tests: one bf16 rounding of the output plus 2e-3 absolute); a strided kv (columns of a wider matrix); and row b of
    a batch of 16 equals the batch-of-1 result bit for bit."""
    g = torch.Generator().manual_seed(200 + dh)
    H = 12 if dh == 64 else 4
    D = H * dh
    for n in POOL_N:
        B = 16
        q = torch.randn(D, generator=g) * 1.5
        wide = bf(torch.randn(B * n, 2 * D + 64, generator=g)).cuda()  # ldkv = 2D + 64: the k | v columns of a wider matrix
        kv = wide[:, : 2 * D]
        out = ops.attention_pool(q.cuda(), kv, B, n, H, dh)
        ref = _pool_ref(q.cuda(), kv, B, n, H, dh)
        err = (out.float() - ref).abs()
        bound = 2e-3 + BF16_EPS * ref.abs()
        assert torch.isfinite(out.float()).all() and (err <= bound).all(), (dh, n, err.max().item())
        for b in (0, 7, 15):
            one = ops.attention_pool(q.cuda(), wide[b * n:(b + 1) * n, : 2 * D], 1, n, H, dh)
            assert torch.equal(one[0], out[b]), f"row {b} depends on the batch (dh {dh}, n {n})"
        dense = ops.attention_pool(q.cuda(), kv.contiguous(), B, n, H, dh)
        assert torch.equal(dense, out), "the row stride of kv must not change the bits"
