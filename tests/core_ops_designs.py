"""Designed inputs and derived bounds for the core operators (vdr_op_linear's activation epilogues, vdr_op_layernorm),
with fp32 torch restatements of the device formulas of csrc/vdr_dev.h and csrc/rowops.hip.  No GPU, no libvdr: the CPU
tests evaluate the designs with the restatements, the GPU tests launch them.

SwiGLU design (swiglu_design).  The packed weight of the epilogue holds, per block of 64 rows, 32 gate rows then 32
value rows; output column j = 32 b + t pairs packed rows 64 b + t (gate) and 64 b + 32 + t (value).
  gate pre-activation   -128 + 160 * bit(j, m % 10)  in {+32, -128}: x[m, m % 10] = 1 against Wg[j, c] = 160 * bit c of
                        (j + 1), bias -128.  silu(a) = a * rcp(1 + exp2(-a log2 e)): at +32 exp2(-46.2) = 1.3e-14 is
                        below half an ulp of 1, so silu = 32 * rcp(1) = 32; at -128 exp2(+184.7) = inf, rcp(inf) = 0, so
                        silu = -0.
  value pre-activation  an integer with |u| <= 7: three +-1 entries of x (columns >= 10) against Wu in [-2, 2], plus an
                        integer bias in [-1, 1].
Every output is 32 u or +-0: an integer of magnitude <= 224, exact in bf16.  The only assumption about the hardware is
rcp(1.0) == 1.0.

Saturated-GELU design (gelu_design).  Pre-activation W[j, m % K] + b[j] = an integer in [8, 199]; each of the three GELU
forms returns a value that rounds to that integer in bf16 (checked on the CPU for every integer of the range).

LayerNorm bound (ln_bound).  See its docstring.
"""
import math

import torch

LOG2E = 1.44269504088896341
U = 2.0 ** -24  # unit roundoff of fp32 (half an ulp of 1)


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


# ---- fp32 restatements of csrc/vdr_dev.h --------------------------------------------------------------------------------
def silu_f32(a: torch.Tensor, rcp_one: float = 1.0) -> torch.Tensor:
    """a * rcp(1 + exp2(-a log2 e)) in fp32; rcp_one: the value the device's rcp returns for 1.0"""
    a = a.float()
    d = _f(1.0) + torch.exp2(-a * _f(LOG2E))
    r = torch.where(d == 1.0, _f(rcp_one), _f(1.0) / d)
    return a * r


def x_sigmoid_f32(x, e2, rcp_one: float = 1.0):
    d = _f(1.0) + torch.exp2(e2)
    return x * torch.where(d == 1.0, _f(rcp_one), _f(1.0) / d)


def quick_gelu_f32(x, rcp_one: float = 1.0):
    x = x.float()
    return x_sigmoid_f32(x, x * _f(-1.702 * LOG2E), rcp_one)


def gelu_tanh_f32(x, rcp_one: float = 1.0):
    x = x.float()
    a = _f(-2.0 * 0.7978845608028654 * LOG2E)
    b = (a * _f(0.044715)).float()
    return x_sigmoid_f32(x, x * (x * x * b + a), rcp_one)


def gelu_erf_f32(x):
    """max(x, 0) - a 2^Q(a), a = min(|x|, 5.7), Q the degree-6 polynomial of gelu_erf (fma steps written as mul + add:
    the difference is below the saturation margin the design relies on)"""
    x = x.float()
    a = torch.minimum(x.abs(), _f(5.7))
    q = _f(2.480073296e-05) * a + _f(-6.399250922e-04)
    for c in (7.365777341e-03, -5.164207073e-02, -4.607286841e-01, -1.150403490e+00, -1.000050145e+00):
        q = q * a + _f(c)
    return torch.clamp(x, min=0.0) - a * torch.exp2(q)


GELU_FORMS = {"gelu": gelu_erf_f32, "quick_gelu": quick_gelu_f32, "gelu_tanh": gelu_tanh_f32}
GELU_RANGE = (8, 199)  # pre-activation integers of gelu_design


# ---- SwiGLU -------------------------------------------------------------------------------------------------------------
GATE_COLS = 10  # x columns 0..9 select the gate pattern, columns >= 10 carry the value


def swiglu_design(M: int, N: int, K: int):
    """x [M, K], packed W [N, K], packed bias [N] (fp32, all bf16-exact integers) and the gate bits [M, N / 2]."""
    assert N % 64 == 0 and K % 64 == 0 and K >= 64 and N // 2 + 1 < (1 << GATE_COLS)
    F = N // 2
    m = torch.arange(M)
    x = torch.zeros(M, K)
    x[m, m % GATE_COLS] = 1.0
    span = K - GATE_COLS
    for i in range(3):
        x[m, GATE_COLS + (m * 3 + i * 17) % span] = torch.where((m + i) % 2 == 0, 1.0, -1.0)
    j = torch.arange(F)
    k = torch.arange(K)
    bits = (((j + 1)[:, None] >> torch.arange(GATE_COLS)[None, :]) & 1).float()  # [F, 10]
    Wg = torch.zeros(F, K)
    Wg[:, :GATE_COLS] = 160.0 * bits
    Wu = (((j[:, None] * 31 + k[None, :] * 17 + (j[:, None] * k[None, :]) % 5) % 5) - 2).float()
    Wu[:, :GATE_COLS] = 0.0
    bg = torch.full((F,), -128.0)
    bu = ((j * 7) % 3 - 1).float()
    # pack: block b of 64 rows = gate rows of outputs 32 b .. 32 b + 31, then their value rows
    W = torch.stack([Wg.view(F // 32, 32, K), Wu.view(F // 32, 32, K)], dim=1).reshape(N, K)
    bias = torch.stack([bg.view(F // 32, 32), bu.view(F // 32, 32)], dim=1).reshape(N)
    gate_bit = bits[:, m % GATE_COLS].t().bool()  # [M, F]
    return x, W, bias, gate_bit


def swiglu_expected(x, W, bias, gate_bit):
    """The integers the design promises: 32 u where the gate is +32, zero (of either sign) elsewhere."""
    M, K = x.shape
    N = W.shape[0]
    Wu = W.view(N // 64, 2, 32, K)[:, 1].reshape(N // 2, K)
    bu = bias.view(N // 64, 2, 32)[:, 1].reshape(N // 2)
    u = x.double() @ Wu.double().t() + bu.double()
    assert u.abs().max() <= 7
    return torch.where(gate_bit, 32.0 * u, torch.zeros_like(u)).float()


def swiglu_eval(x, W, bias, bug: str = None, rcp_one: float = 1.0):
    """The epilogue restated in fp32 (gemm_epi.h: value half read at n + 32, output column (n >> 6) * 32 + (n & 31)), with
    one planted bug: "swap_halves", "pair_shift_32", "plain_column", "drop_bias_half"."""
    M, K = x.shape
    N = W.shape[0]
    acc = (x.double() @ W.double().t()).float()  # integer sums: exact
    b = bias.float().clone()
    blk = N // 64
    g_idx = (torch.arange(blk)[:, None] * 64 + torch.arange(32)[None, :]).reshape(-1)  # packed column n of each output
    u_idx = g_idx + 32
    if bug == "swap_halves":
        g_idx, u_idx = u_idx, g_idx
    if bug == "pair_shift_32":
        u_idx = (g_idx + 64) % N  # the block after the right one
    accb = acc + b
    if bug == "drop_bias_half":
        u = acc[:, u_idx]
    else:
        u = accb[:, u_idx]
    v = silu_f32(accb[:, g_idx], rcp_one) * u
    out = torch.full((M, N), float("nan"))
    n = torch.arange(blk)[:, None] * 64 + torch.arange(32)[None, :]
    oc = ((n >> 6) * 32 + (n & 31)).reshape(-1)
    if bug == "plain_column":
        oc = n.reshape(-1)  # the un-permuted column of the other epilogues (the same column while N == 64)
    out[:, oc] = v
    return out[:, :N // 2].to(torch.bfloat16)


SWIGLU_BUGS = ("swap_halves", "pair_shift_32", "plain_column", "drop_bias_half")


# ---- saturated GELU -----------------------------------------------------------------------------------------------------
def gelu_design(M: int, N: int, K: int):
    """x [M, K] one-hot rows, W [N, K], bias [N] and the expected pre-activation = output integers [M, N] in GELU_RANGE."""
    m, j, k = torch.arange(M), torch.arange(N), torch.arange(K)
    x = torch.zeros(M, K)
    x[m, m % K] = 1.0
    W = ((k[None, :] * 37 + j[:, None] * 11) % 188).float()
    bias = (8 + j % 5).float()
    want = W[:, m % K].t() + bias[None, :]
    assert want.min() >= GELU_RANGE[0] and want.max() <= GELU_RANGE[1]
    return x, W, bias, want


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 8, 64, 252, 256, 260, 764, 1020, 1024, 1028, 2044, 2048)
LN_ROWS = (1, 3, 4, 5, 9)
LN_RSQRT_ULP = 2  # rsqrtf is allowed 2 ulp (the hardware instruction is good to 1)


def ln_depth(D: int) -> int:
    """Most additions any one term of a row sum passes through in rowops.hip: a lane adds its 4 columns of each of the
    ceil(D / 256) passes one after the other, then 6 shuffle levels combine the 64 lanes."""
    return 4 * ((D + 255) // 256) + 6


def ln_ref64(x, gamma, beta, eps):
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def ln_bound(x, gamma, beta, eps, out_dtype):
    """Entry-wise bound on |kernel - float64 LayerNorm| for inputs x (already rounded to the input type: the conversion to
    fp32 is exact), from the kernel's arithmetic.  u = 2^-24, d = ln_depth(D), A = mean |x| of the row, c = x - mean,
    s = 1 / sqrt(var + eps), o = c s g + b, all in exact arithmetic:

      mean      a sum of depth d, times the rounded 1 / D:          |dmu| <= (d + 2) u A
      centring  one subtraction: c^ = (c - dmu)(1 + u)
      variance  squares (1 rounding each), a sum of depth d, times the rounded 1 / D, and sum (c - dmu)^2 = sum c^2 +
                D dmu^2 because sum c = 0:                          var^ + eps = (var + eps)(1 + ev),
                                                                     ev <= (d + 5) u + dmu^2 / (var + eps) + u  (the + eps)
      rsqrtf    LN_RSQRT_ULP ulp = 2 LN_RSQRT_ULP u:                s^ = s (1 + es), es <= ev / 2 + 2 LN_RSQRT_ULP u
      affine    two multiplications and one addition (or one fma):
                |o^ - o| <= |g| s |dmu| + |c s g| (es + 3 u) + u |o|
      store     bf16: one more rounding to nearest, 2^-8 |o^| (the unit roundoff of 8 significand bits); fp32: none.
    Second-order terms are covered by the factor (1 + 2^-10) on the whole.  Nothing here is fitted to the kernel's output.
    """
    x, g, b = x.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    d = ln_depth(D)
    A = x.abs().mean(dim=-1, keepdim=True)
    mu = x.mean(dim=-1, keepdim=True)
    c = x - mu
    var = (c ** 2).mean(dim=-1, keepdim=True)
    s = 1.0 / torch.sqrt(var + eps)
    o = c * s * g + b
    dmu = (d + 2) * U * A
    ev = (d + 6) * U + dmu ** 2 / (var + eps)
    es = ev / 2 + 2 * LN_RSQRT_ULP * U
    bound = g.abs() * s * dmu + (c * s * g).abs() * (es + 3 * U) + U * o.abs()
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (o.abs() + bound)
    return bound * (1 + 2.0 ** -10)


def _wave_layout(x):
    """x [rows, D] fp32 -> [rows, NP, 64, 4] zero padded: lane l owns columns k*256 + 4l .. 4l + 3 of pass k"""
    rows, D = x.shape
    NP = (D + 255) // 256
    v = torch.zeros(rows, NP * 256, dtype=torch.float32)
    v[:, :D] = x
    return v.view(rows, NP, 64, 4)


def _wave_sum(t):
    """the kernel's order: per lane pass by pass, element by element, then a butterfly over the 64 lanes; t [rows, NP, 64, 4]"""
    s = torch.zeros(t.shape[0], 64, dtype=torch.float32)
    for k in range(t.shape[1]):
        for e in range(4):
            s = s + t[:, k, :, e]
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ off]
    return s[:, :1]


def ln_two_pass_fp32(x, gamma, beta, eps, out_dtype):
    """Plain fp32 emulation of layernorm_kernel: two-pass mean and variance in the kernel's summation order."""
    x = x.float()
    D = x.shape[-1]
    v = _wave_layout(x)
    invD = _f(1.0) / _f(float(D))
    mean = _wave_sum(v) * invD
    dv = _wave_layout(x - mean)
    dv.view(x.shape[0], -1)[:, D:] = 0.0
    rstd = torch.rsqrt(_wave_sum(dv * dv) * invD + _f(eps))
    return ((x - mean) * rstd * gamma.float() + beta.float()).to(out_dtype)


def ln_one_pass_fp32(x, gamma, beta, eps, out_dtype):
    """The rewrite the offset case guards against: var = E[x^2] - mean^2 in fp32."""
    x = x.float()
    D = x.shape[-1]
    v = _wave_layout(x)
    invD = _f(1.0) / _f(float(D))
    mean = _wave_sum(v) * invD
    var = _wave_sum(v * v) * invD - mean * mean
    rstd = torch.rsqrt(torch.clamp(var, min=0.0) + _f(eps))
    return ((x - mean) * rstd * gamma.float() + beta.float()).to(out_dtype)


def ln_inputs(D: int, rows: int, in_dtype, seed: int = 0):
    g = torch.Generator().manual_seed(1000 * D + rows + seed)
    x = (torch.randn(rows, D, generator=g) * 1.7 + 0.3).to(in_dtype)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    return x, gamma, beta


def ln_offset_case(rows: int = 9, D: int = 1024, seed: int = 7):
    """fp32 rows of 1000 + N(0, 1): two-pass statistics keep the bound, E[x^2] - mean^2 in fp32 cannot."""
    g = torch.Generator().manual_seed(seed)
    x = 1000.0 + torch.randn(rows, D, generator=g)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    return x, gamma, beta


def worst_ratio(got, x, gamma, beta, eps, out_dtype) -> float:
    err = (got.double() - ln_ref64(x, gamma, beta, eps)).abs()
    r = err / ln_bound(x, gamma, beta, eps, out_dtype)
    return float(r.max()) if torch.isfinite(got.double()).all() else math.inf
