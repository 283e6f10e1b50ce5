"""GPU: the 2-D RoPE operators (csrc/rope.hip) through the C ABI -- vdr_op_rope2d_table against a numpy float64 evaluation,
vdr_op_rope2d on designed inputs (exact to the bit) and on random inputs against float64 within a derived bound.

Shapes: head dim 32 / 64 / 128 (every instantiation), 1 and 3 heads, batch 2, a 3 x 5 grid (non-square: swapping y and x
shows) behind 0, 1 or 5 prefix rows (the odd prefixes misalign the patch rows), so at most 20 tokens.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GH, GW, BATCH, THETA = 3, 5, 2, 100.0
CASES = [(dh, heads, prefix) for dh in (32, 64, 128) for heads in (1, 3) for prefix in (0, 1, 5)]


def _table64(gh, gw, dh, theta):
    """the definition in numpy float64: (angles, cos, sin) [gh*gw, dh/2]"""
    q = dh // 4
    inv = np.float64(theta) ** (-4.0 * np.arange(q, dtype=np.float64) / dh)
    cy = 2.0 * (np.arange(gh, dtype=np.float64) + 0.5) / gh - 1.0
    cx = 2.0 * (np.arange(gw, dtype=np.float64) + 0.5) / gw - 1.0
    a = np.zeros((gh, gw, 2 * q))
    a[:, :, :q] = 2.0 * np.pi * cy[:, None, None] * inv[None, None, :]
    a[:, :, q:] = 2.0 * np.pi * cx[None, :, None] * inv[None, None, :]
    a = a.reshape(gh * gw, 2 * q)
    return a, np.cos(a), np.sin(a)


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("grid,theta", [((GH, GW), 100.0), ((14, 14), 100.0), ((37, 50), 10000.0)])
def test_table_matches_the_float64_definition(dh, grid, theta):
    """|table - float64 value| <= 2^-23: one fp32 ulp at 1.0, i.e. the final rounding (half an ulp) plus whatever the
    device's fp64 cos / sin, which are not guaranteed correctly rounded, add."""
    from vdr import ops
    from vdr.weights import rope2d_table
    cos, sin = ops.rope2d_table(grid, dh, theta)
    assert cos.shape == sin.shape == (grid[0] * grid[1], dh // 2) and cos.dtype == torch.float32
    _, c64, s64 = _table64(grid[0], grid[1], dh, theta)
    ec = np.abs(cos.cpu().numpy().astype(np.float64) - c64).max()
    es = np.abs(sin.cpu().numpy().astype(np.float64) - s64).max()
    print(f"dh {dh} grid {grid} theta {theta}: max |cos - f64| {ec:.3e}  max |sin - f64| {es:.3e}  (2^-23 = {2.0 ** -23:.3e})")
    assert ec <= 2.0 ** -23 and es <= 2.0 ** -23
    # the host statement the restatement uses (tests/dinov3_ref.py) obeys the same bound
    hc, hs = rope2d_table(grid, dh, theta)
    assert np.abs(hc.numpy().astype(np.float64) - c64).max() <= 2.0 ** -23 and np.abs(hs.numpy().astype(np.float64) - s64).max() <= 2.0 ** -23
    if grid == (GH, GW):  # y and x are told apart: the two halves of a row differ, and rows of one y share the first half
        c = cos.cpu().reshape(GH, GW, dh // 2)
        assert torch.equal(c[:, 0, :dh // 4], c[:, GW - 1, :dh // 4]) and not torch.equal(c[0, :, dh // 4:], c[0, :, :dh // 4])
        assert torch.equal(c[0, :, dh // 4:], c[GH - 1, :, dh // 4:]) and not torch.equal(c[0, 0], c[1, 0])  # (rows 0 and GH - 1: cy = -/+ 2/3, the same cosines)


def _distinct_buffer(rows, cols, seed):
    """bf16 [rows, cols], every element a different finite non-zero value (moderate exponents: no overflow in a rotation)"""
    exps = torch.arange(20, 235, dtype=torch.int32)
    pats = ((exps[:, None] << 7) | torch.arange(128, dtype=torch.int32)[None, :]).reshape(-1)
    pats = torch.cat([pats, pats | 0x8000])
    assert rows * cols <= pats.numel()
    perm = torch.randperm(pats.numel(), generator=torch.Generator().manual_seed(seed))[: rows * cols]
    return pats[perm].to(torch.int16).view(torch.bfloat16).reshape(rows, cols)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _split(t, heads, dh):
    """[rows, 3 H dh] -> q, k, v each [rows, H, dh]"""
    q, k, v = t.reshape(t.shape[0], 3, heads, dh).unbind(1)
    return q, k, v


@pytest.mark.parametrize("dh,heads,prefix", CASES)
def test_designed_inputs_are_exact_to_the_bit(dh, heads, prefix):
    from vdr import ops
    n, half = GH * GW, dh // 2
    seq = prefix + n
    x = _distinct_buffer(BATCH * seq, 3 * heads * dh, seed=dh + heads + prefix)
    assert torch.unique(_bits(x).reshape(-1)).numel() == x.numel()
    patch = (torch.arange(BATCH * seq) % seq) >= prefix
    one, zero = torch.ones(n, half, device="cuda"), torch.zeros(n, half, device="cuda")
    # cos = 1, sin = 0: unchanged
    y = ops.rope2d(x.cuda().clone(), BATCH, seq, prefix, heads, dh, one, zero).cpu()
    assert torch.equal(_bits(y), _bits(x))
    # cos = 0, sin = 1: lo' = -hi, hi' = lo
    y = ops.rope2d(x.cuda().clone(), BATCH, seq, prefix, heads, dh, zero, one).cpu()
    want = x.clone()
    for src, dst in zip(_split(x, heads, dh)[:2], _split(want.reshape(-1, 3 * heads * dh), heads, dh)[:2]):
        lo, hi = src[..., :half], src[..., half:]
        dst[patch, :, :half] = (-hi)[patch]
        dst[patch, :, half:] = lo[patch]
    assert torch.equal(_bits(y), _bits(want))
    # the real table: prefix rows and every v column come back bit-identical, q and k of the patch rows move
    cos, sin = ops.rope2d_table((GH, GW), dh, THETA, device="cuda")
    y = ops.rope2d(x.cuda().clone(), BATCH, seq, prefix, heads, dh, cos, sin).cpu()
    assert torch.equal(_bits(y[~patch]), _bits(x[~patch]))
    assert torch.equal(_bits(_split(y, heads, dh)[2]), _bits(_split(x, heads, dh)[2]))
    for a, b in zip(_split(y, heads, dh)[:2], _split(x, heads, dh)[:2]):
        # (not all of them: the middle row / column of the 3 x 5 grid has coordinate 0, i.e. angle 0 in its half, and the
        # lowest frequencies turn by less than a bf16 ulp)
        assert (_bits(a[patch]) != _bits(b[patch])).float().mean() > 0.3


@pytest.mark.parametrize("dh,heads,prefix", CASES)
def test_random_inputs_against_float64_and_batch_independence(dh, heads, prefix):
    """|out - exact| <= 1/2 ulp_bf16(exact) + 2^-22 (|lo| + |hi|): the one bf16 rounding, plus three fp32 roundings (two
    products and their sum or difference, each of magnitude <= |lo| + |hi|: 3 x 2^-24), doubled for margin.  exact: float64 on
    the same bf16 inputs and fp32 table."""
    from vdr import ops
    n, half = GH * GW, dh // 2
    seq = prefix + n
    g = torch.Generator().manual_seed(100 + dh + heads + prefix)
    x = torch.randn(BATCH * seq, 3 * heads * dh, generator=g).to(torch.bfloat16)
    cos, sin = ops.rope2d_table((GH, GW), dh, THETA, device="cuda")
    y = ops.rope2d(x.cuda().clone(), BATCH, seq, prefix, heads, dh, cos, sin).cpu()
    c64, s64 = cos.cpu().double()[:, None, :], sin.cpu().double()[:, None, :]
    patch = (torch.arange(BATCH * seq) % seq) >= prefix
    worst = 0.0
    for got, src in zip(_split(y, heads, dh)[:2], _split(x, heads, dh)[:2]):
        got = got[patch].double().reshape(BATCH, n, heads, dh)
        src = src[patch].double().reshape(BATCH, n, heads, dh)
        lo, hi = src[..., :half], src[..., half:]
        exact = torch.cat([lo * c64 - hi * s64, hi * c64 + lo * s64], dim=-1)
        mag = (lo.abs() + hi.abs()).repeat(1, 1, 1, 2)
        ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -126))) - 7)
        bound = 0.5 * ulp + 2.0 ** -22 * mag
        err = (got - exact).abs()
        worst = max(worst, (err / bound).max().item())
        assert (err <= bound).all(), (err / bound).max().item()
    print(f"dh {dh} heads {heads} prefix {prefix}: worst |out - exact| / bound = {worst:.3f}")
    # a row's bits at batch 1 and inside batch 2
    for b in range(BATCH):
        one = ops.rope2d(x[b * seq:(b + 1) * seq].cuda().clone(), 1, seq, prefix, heads, dh, cos, sin).cpu()
        assert torch.equal(_bits(one), _bits(y[b * seq:(b + 1) * seq]))
