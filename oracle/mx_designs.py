"""Designed inputs for the MX-fp8 path, the checks that go with them, and a torch model of its arithmetic.

TEST INFRASTRUCTURE ONLY (never imported by the product package).

The MX-fp8 path (csrc/mx.hip, gemm_mx.hip, the EPI_*_MX branch of gemm_epi.h) has three producers of MX tensors -- the
plain quantiser, LayerNorm to MX, the re-quantising GEMM epilogue -- and one consumer, the block-scaled GEMM.
tests/test_mx_exact_gpu.py runs the constructions below through the kernels and compares raw payload and scale bytes;
tests/test_mx_gates_cpu.py runs them through `model_*` with and without injected bugs, to show that each check rejects
the bugs it is meant to catch.

  encode / place_scales  the raw encoding: payload bytes (torch float8_e4m3fn viewed as uint8) and e8m0 scale bytes at
                         the offsets of mx_scale_offsets (the single restatement of the device layout of csrc/mx.hip)
  edge_blocks            one edge of the quantiser per 32-element block (EDGE_NAMES lists them)
  integer_case           the small-integer GEMM with block shifts in {0, 1, 2}
  wide_scale_case        the same with block exponents u(kb) + alpha(m) and -u(kb) + beta(n), u in [-40, 40]
  epilogue_case          bias / GELU / residual / SwiGLU on integer data: bf16- and MX-exact (see below)
  ln_mx_case             designed LayerNorm rows; check_mx_bytes excludes only what fp32 rounding noise can move

The exact sets of the fused activations rest on csrc/vdr_dev.h:
  gelu_erf(v) = fmaf(-a, exp2(Q(a)), max(v, 0)), a = min(|v|, 5.7)          (vdr_dev.h gelu_erf, gelu_erf2)
    v = 0      a = 0: fmaf(-0, 2^Q(0), 0) = +0
    v >= 8     a = 5.7: the subtrahend 5.7 * 2^Q(5.7) = 3.4e-8 is below half an fp32 ulp of 8 (4.8e-7): exactly v
    v <= -8    max(v, 0) = 0: -3.4e-8 (GELU_NEG_TAIL), which an e4m3 block holding a value >= 8 rounds to -0
  silu(x) = x * rcp(1 + exp2(-x * log2 e))                                   (vdr_dev.h silu)
    x = 0      0 * rcp(2) = +0
    x >= 32    exp2(-46.2) = 1.2e-14 is below half an ulp of 1: rcp(1) = 1, exactly x
    x <= -128  exp2(184.7) = +inf: rcp(inf) = 0, x * 0 = -0
  so GELU outputs are integers, +0 or the tail, SwiGLU outputs silu(gate) * u are integers or signed zeros (the sign is
  that of the IEEE product), and the expected MX bytes are the oracle quantiser of exact values: no exclusions.

NOISE_ULPS.  check_mx_bytes excludes an element only where the float64 reference, scaled, lies within `noise` of an e4m3
rounding midpoint, and a block only where its maximum / 448 lies within `noise` of a power of two.  noise = NOISE_ULPS
fp32 ulps of S = |(x - mean) rstd gamma| + |beta|, the magnitudes the last fp32 operation rounds at.  Measured on the
CPU (tests/test_mx_gates_cpu.py::test_noise_constant_covers_the_fp32_model re-measures it): the largest difference
between the float64 LayerNorm and the fp32 model `model_ln` over ln_mx_case at D in {32, 96, 512, 544, 1536, 2048}, 130
and 1 / 5 / 130 rows, is 0.7502 ulp32(S) (MEASURED_ULPS); times 4, because the kernel sums a row in another order than the model (and
v_rsq_f32 is good to 1 ulp): NOISE_ULPS = 3.0008.  The fp32 model and the float64 reference disagree on no byte of any of
these cases, and no element falls inside the noise: the cap of 1 element in 2000 is a backstop.
"""
from __future__ import annotations

import torch

from . import mx_oracle as mx
from .ln_fold_designs import bf16_round, cycled_rows

BLOCK = 32
MEASURED_ULPS = 0.7502  # largest |float64 - fp32 model| over the designed LayerNorm cases, in ulp32(S)
NOISE_ULPS = 4 * MEASURED_ULPS
MAX_EXCLUDED_FRAC = 1.0 / 2000
EPS = 1e-6
GELU_Q = (2.480073296e-05, -6.399250922e-04, 7.365777341e-03, -5.164207073e-02, -4.607286841e-01, -1.150403490e+00,
          -1.000050145e+00)  # the polynomial of csrc/vdr_dev.h gelu_erf, highest degree first


def _gelu_neg_tail() -> float:
    q = 0.0
    for c in GELU_Q:
        q = q * 5.7 + c
    return -5.7 * 2.0 ** q


GELU_NEG_TAIL = _gelu_neg_tail()  # gelu_erf(v <= -5.7) = -5.7 * 2^Q(5.7) = -3.4e-8
BUGS_QUANT = ("floor_exp", "trunc", "ties_away", "ftz", "amax8", "amax16", "pair_swapped", "rows_pad_as_rows",
              "neighbour_scale")
BUGS_GEMM = ("neighbour_scale", "pair_swapped", "rows_pad_as_rows", "scales_exchanged")
BUGS_EPI = ("amax_before_act", "no_fold", "amax8", "amax16", "floor_exp", "trunc")
BUGS_LN = ("unbiased", "eps_outside")


# ---- layout -------------------------------------------------------------------------------------------------------
def mx_rows_pad(rows):
    return (rows + 255) // 256 * 256


def mx_scale_slot(rows: torch.Tensor) -> torch.Tensor:
    """row -> position of its scale byte inside one block plane: (r, r + 32) pairs inside every 64-row group"""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    return (rows & ~63) + 2 * (rows & 31) + ((rows >> 5) & 1)


def mx_scale_offsets(rows_total, rows, K):
    """Byte offsets, [len(rows), K / 32], of the e8m0 scales of the given rows inside the scale array of an MX tensor of
    rows_total rows (include/vdr.h: s[K/32][rows_pad], rows_pad = rows_total rounded up to 256; inside every 64-row group
    rows are stored as (r, r + 32) pairs)."""
    return torch.arange(K // 32)[None, :] * mx_rows_pad(rows_total) + mx_scale_slot(rows)[:, None]


def _offsets(rows: int, K: int, bug: str | None = None) -> torch.Tensor:
    r = torch.arange(rows)
    if bug == "pair_swapped":
        slot = (r & ~63) + 2 * (r & 31) + 1 - ((r >> 5) & 1)
    else:
        slot = mx_scale_slot(r)
    stride = rows if bug == "rows_pad_as_rows" else mx_rows_pad(rows)
    return torch.arange(K // 32)[None, :] * stride + slot[:, None]


def place_scales(sb: torch.Tensor, fill: int = 0, bug: str | None = None) -> torch.Tensor:
    """scale bytes [rows, K/32] -> the flat device array (every other byte `fill`)"""
    rows, nb = sb.shape
    flat = torch.full((mx_rows_pad(rows) * nb,), fill, dtype=torch.uint8)
    flat[_offsets(rows, nb * 32, bug).reshape(-1)] = sb.reshape(-1)
    return flat


def gather_scales(flat: torch.Tensor, rows: int, K: int, bug: str | None = None) -> torch.Tensor:
    return flat.cpu()[_offsets(rows, K, bug).reshape(-1)].reshape(rows, K // 32)


def unwritten_mask(rows: int, K: int) -> torch.Tensor:
    """True at every byte of the flat scale array that is no valid (row, block) slot"""
    m = torch.ones(mx_rows_pad(rows) * (K // 32), dtype=torch.bool)
    m[mx_scale_offsets(rows, torch.arange(rows), K).reshape(-1)] = False
    return m


# ---- raw encoding -------------------------------------------------------------------------------------------------
def exact_scale_exponent(amax: torch.Tensor) -> torch.Tensor:
    """ceil(log2(amax / 448)) clamped to [-126, 126] by exact arithmetic: amax = m 2^x with m in [1/2, 1) and
    448 = 7/8 * 2^9, so the logarithm is x - 9 + log2(m / (7/8)), whose ceiling is x - 9 for m <= 7/8 and x - 8 above.
    Independent of the fp32 product amax * fl(1 / 448) the kernels and mx_oracle.scale_exponent use; zero gives -126"""
    m, x = torch.frexp(amax.double())
    e = x.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)
    e = torch.where(amax == 0, torch.full_like(e, -126), e)
    return e.clamp(-126, 126).to(torch.int32)


def encode(x: torch.Tensor, ignore_nan: bool = False):
    """x [rows, K] -> (payload uint8 [rows, K], scale bytes uint8 [rows, K/32]) by the oracle quantiser"""
    q, e = mx.mx_quantize(x, ignore_nan=ignore_nan)
    return q.view(torch.uint8), (e + 127).to(torch.uint8)


def decode(q: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """payload bytes [rows, K], scale bytes [rows, K/32] -> float64 values"""
    v = q.view(torch.float8_e4m3fn).to(torch.float32).double().reshape(q.shape[0], -1, BLOCK)
    return (v * torch.ldexp(torch.ones_like(v[..., 0]), sb.to(torch.int32) - 127)[..., None]).reshape(q.shape)


def e4m3_round(y: torch.Tensor, mode: str = "rne") -> torch.Tensor:
    """|y| <= 448 (fp32 or float64 values) to the e4m3 grid, returned as payload bytes.  mode "rne" | "trunc" |
    "ties_away" | "ftz" (round to nearest even, subnormal results flushed to zero); written in integer steps of the grid so
    that the wrong roundings can be modelled, and checked against torch's cast in the gates"""
    y = y.double()
    a = y.abs()
    ex = torch.floor(torch.log2(a)).clamp(min=-6.0)
    ex = torch.where(a == 0, torch.full_like(ex, -6.0), ex)
    step = torch.exp2(ex - 3)
    f = a / step  # exact: a power-of-two scaling
    if mode == "trunc":
        n = torch.floor(f)
    elif mode == "ties_away":
        n = torch.floor(f + 0.5)
    else:
        n = torch.round(f)  # half to even
    v = n * step
    if mode == "ftz":
        v = torch.where(v < 2.0 ** -6, torch.zeros_like(v), v)
    v = torch.minimum(v, torch.full_like(v, 448.0))
    v = torch.where(torch.isnan(y), y, torch.copysign(v, y))
    return v.float().to(torch.float8_e4m3fn).view(torch.uint8)


def model_quantize(x: torch.Tensor, bug: str | None = None, ignore_nan: bool = True):
    """the quantiser kernels' arithmetic: (payload uint8 [rows, K], flat scale array).  Bugs: BUGS_QUANT"""
    x = x.float()
    rows, K = x.shape
    grp = {"amax8": 8, "amax16": 16}.get(bug, BLOCK)
    xg = x.reshape(rows, K // grp, grp)
    a = xg.abs()
    if ignore_nan:
        a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    amax = a.amax(-1)
    e = mx.scale_exponent(amax, ignore_nan)
    if bug == "floor_exp":
        t = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).contiguous()
        e = (((t.view(torch.int32) >> 23) & 255) - 127).clamp(-126, 126)
    y = xg * torch.ldexp(torch.ones_like(amax), -e)[..., None]
    mode = bug if bug in ("trunc", "ties_away", "ftz") else "rne"
    q = e4m3_round(y.clamp(-448.0, 448.0) if bug == "floor_exp" else y, mode).reshape(rows, K)
    sb = (e.reshape(rows, K // BLOCK, BLOCK // grp)[..., 0] + 127).to(torch.uint8)  # the first lane of a quad stores
    if bug == "neighbour_scale":
        sb = torch.roll(sb, 1, 1)
    return q, place_scales(sb, bug=bug)


# ---- designed inputs: the quantiser -------------------------------------------------------------------------------
def _bf16_step(x: torch.Tensor, n: int) -> torch.Tensor:
    """the bf16 value n steps away from zero (n < 0: towards zero) of bf16-exact positive x"""
    return (x.to(torch.bfloat16).view(torch.int16) + n).view(torch.bfloat16).float()


def _edge_list():
    """[(name, 32 float values)], every value bf16-exact"""
    out = []
    P = lambda e: 2.0 ** e  # noqa: E731
    # subnormal sweep under a maximum of exactly 448 * 2^k (scaled by 2^-k: the ties (2m + 1) 2^-10, their bf16
    # neighbours either side, and the subnormals m 2^-9 themselves), and under one bf16 step above / below it (446 and
    # 450: the step at 448 is 2), where the scale exponent is k and k + 1
    ties = torch.tensor([(2 * m + 1) * P(-10) for m in range(8)])
    sweep = torch.cat([_bf16_step(ties, -1), ties, _bf16_step(ties, 1), torch.tensor([m * P(-9) for m in range(1, 8)])])
    for k in (-126, -110, -20, -1, 0, 3, 40, 118):
        for name, top in (("max448", 448.0), ("max450", 450.0), ("max446", 446.0)):
            if k == -126:  # (the sweep would need values below the smallest bf16 subnormal)
                body = torch.tensor([2.0 ** (-133 + (i % 8)) * (1 + i // 8) for i in range(31)])
            else:
                body = sweep * P(k)
            out.append((f"{name}_k{k}", torch.cat([torch.tensor([top * P(k)]), body])))
    # round-to-nearest-even ties in the normal range: 17 .. 31 and 34 .. 62 under a maximum of 448 (scaled by 1), the
    # bf16 neighbours of the first eight
    odd = torch.tensor([17.0, 19, 21, 23, 25, 27, 29, 31])
    out.append(("normal_ties", torch.cat([torch.tensor([448.0]), odd, odd * 2, _bf16_step(odd, 1), _bf16_step(odd[:7], -1)])))
    out.append(("normal_ties_hi", torch.cat([torch.tensor([448.0]), odd * 8, odd * 4, odd[:6] * 16, _bf16_step(odd[:2] * 16, 1), odd[:7] * P(-3)])))
    # ratio sweep: 2^-1 .. 2^-20 of the maximum (2^-17: the subnormal 2^-9, 2^-18: the flush tie, below: zero), 1.5 x
    for k in (-60, 0, 9, 77):
        r = torch.tensor([P(-i) for i in range(1, 21)] + [1.5 * P(-i) for i in range(8, 19)])
        out.append((f"ratio_k{k}", torch.cat([torch.tensor([1.0]), r]) * P(k)))
    out.append(("zeros", torch.zeros(32)))
    out.append(("neg_zeros", -torch.zeros(32)))
    out.append(("mixed_zeros", torch.cat([torch.tensor([0.0, -0.0] * 15), torch.tensor([-P(-40), -0.0])])))
    # below the lower clamp (maximum < 448 * 2^-126 = 1.75 * 2^-118): the scale stays 2^-126, bf16-subnormal inputs
    sub = torch.tensor([P(-133) * (1 + (i % 127)) for i in range(0, 31 * 9, 9)])  # bf16 subnormals: multiples of 2^-133
    out.append(("clamp_max_2^-120", torch.cat([torch.tensor([P(-120)]), sub])))
    out.append(("clamp_max_subnormal", torch.cat([torch.tensor([P(-127)]), torch.full((31,), P(-133))])))
    out.append(("clamp_min_subnormal", torch.cat([torch.tensor([P(-133)]), torch.zeros(31)])))
    out.append(("clamp_448*2^-127", torch.cat([torch.tensor([448.0 * P(-127)]), sub])))
    # near the bf16 maximum (0x7F7F = (2 - 2^-7) 2^127)
    top = (2.0 - P(-7)) * P(127)
    out.append(("bf16_max", torch.cat([torch.tensor([top]), torch.tensor([top * P(-i) for i in range(1, 32)])])))
    out.append(("bf16_max_pair", torch.tensor([top, -top] * 16)))
    # alternating signs with the maximum carried by a negative element
    out.append(("alternating", torch.tensor([(-1.0) ** i * (i + 1) for i in range(31)] + [-448.0])))
    return out


EDGE_NAMES = tuple(n for n, _ in _edge_list())


def edge_blocks(rows: int | None = None, K: int | None = None) -> torch.Tensor:
    """bf16-exact [rows, K]: block (r, kb) is edge (r K/32 + kb) mod len(EDGE_NAMES), with alternating signs (even
    blocks) and rotated by 7 positions per block, so that the maximum visits every lane of the 4-lane quad.  Default
    shape: every edge once, 8 blocks per row"""
    edges = _edge_list()
    if rows is None:
        K = 8 * BLOCK
        rows = -(-len(edges) // 8)
    nb = K // BLOCK
    sign = torch.tensor([(-1.0) ** i for i in range(BLOCK)])
    blocks = []
    for i, (_, v) in enumerate(edges):
        v = v.float()
        assert v.numel() == BLOCK, (edges[i][0], v.numel())
        if i % 2 == 0:
            v = v * sign
        blocks.append(torch.roll(v, (7 * i) % BLOCK))
    idx = torch.arange(rows * nb) % len(blocks)
    x = torch.stack(blocks)[idx].reshape(rows, K)
    assert torch.equal(x.to(torch.bfloat16).float(), x), "edge blocks must be bf16-exact"
    return x


def random_rows(rows: int, K: int, seed: int = 0) -> torch.Tensor:
    """bf16-exact random rows over nine decades (row r scaled by 10^(-5 .. 4))"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * torch.logspace(-5, 4, rows)[:, None]
    return bf16_round(x)


# ---- designed inputs: the GEMM ------------------------------------------------------------------------------------
def _spread(rows: int, K: int, g: torch.Generator, per_row: int = 64) -> torch.Tensor:
    """[rows, K] mask with the same number of ones in every 32-element block of a row, at most per_row in all"""
    nb = K // BLOCK
    cnt = min(BLOCK, max(1, per_row // nb))
    order = torch.rand(rows, nb, BLOCK, generator=g).argsort(-1)
    return (order < cnt).reshape(rows, K)


def integer_case(M: int, N: int, K: int, seed: int = 0):
    """(x, w, ref64): values in {-2 .. 2} * 2^s with a per-(row, block) shift s in {0, 1, 2}, x thinned out to about 48
    non-zeros per row: every product and every partial sum is an integer below 2^15, exact in fp32 in any order, so the
    GEMM must return bf16(ref) bit for bit (one rounding)"""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(0, 3, (M, K // 32, 1), generator=g)
    ws = torch.randint(0, 3, (N, K // 32, 1), generator=g)
    x = (torch.randint(-2, 3, (M, K // 32, 32), generator=g) * (2 ** xs)).reshape(M, K).float()
    w = (torch.randint(-2, 3, (N, K // 32, 32), generator=g) * (2 ** ws)).reshape(N, K).float()
    x = x * (torch.rand(M, K, generator=g) < min(1.0, 48.0 / K))
    ref = x.double() @ w.double().t()
    assert float((x.abs().double() @ w.abs().double().t()).max()) < 2 ** 15
    return x, w, ref


def wide_scale_case(M: int, N: int, K: int, seed: int = 0):
    """(x, w, ref64): x = {-1, 0, 1} 2^(u(kb) + alpha(m)), w = {-2 .. 2} 2^(-u(kb) + beta(n)), u in [-40, 40], alpha and
    beta in {0, 1, 2}; at most 64 non-zero x per row, spread over all blocks: every product is a small integer times
    2^(alpha + beta), |sum| <= 128 * 2^(alpha + beta), bf16-exact.  A scale from the wrong K block is off by 2^(u - u')"""
    g = torch.Generator().manual_seed(seed)
    nb = K // BLOCK
    u = torch.randint(-40, 41, (nb,), generator=g)
    if nb > 1:
        u[0], u[-1] = 40, -40
        u = u - (u == torch.roll(u, 1)).to(u.dtype) * 7  # neighbouring blocks never share u
    alpha = torch.randint(0, 3, (M,), generator=g)
    beta = torch.randint(0, 3, (N,), generator=g)
    xi = torch.randint(0, 2, (M, K), generator=g) * 2 - 1
    xi = (xi * _spread(M, K, g)).reshape(M, nb, BLOCK)
    wi = torch.randint(-2, 3, (N, nb, BLOCK), generator=g)
    x = (xi.double() * torch.exp2((u[None, :] + alpha[:, None]).double())[..., None]).reshape(M, K)
    w = (wi.double() * torch.exp2((-u[None, :] + beta[:, None]).double())[..., None]).reshape(N, K)
    ref = x @ w.t()
    assert torch.equal(bf16_round(x).double(), x) and torch.equal(bf16_round(w).double(), w)
    assert torch.equal(bf16_round(ref).double(), ref) and float(ref.abs().max()) <= 128 * 16
    return x.float(), w.float(), ref


def _sparse_weight(N: int, K: int, g: torch.Generator, nnz: int = 16) -> torch.Tensor:
    """[N, K] of -1 / 0 / +1 with nnz non-zeros per row, one in each of nnz equal stretches of K (every 64-element K
    unit is hit by some row: the position inside the stretch is random)"""
    nnz = min(nnz, K // 4)
    w = torch.zeros(N, nnz, K // nnz)
    pos = torch.randint(0, K // nnz, (N, nnz, 1), generator=g)
    w.scatter_(2, pos, (torch.randint(0, 2, (N, nnz, 1), generator=g) * 2 - 1).float())
    return w.reshape(N, K)


def epilogue_case(kind: str, M: int, N: int, K: int, seed: int = 0):
    """Operands whose fused epilogue is exact in the kernel's own arithmetic.  x in {-1, 0, 1}, W sparse (|x.W| <= 16).
    Returns a dict: x [M, K], w [Nw, K] (SwiGLU: 2 N rows in PyTorch order x1 | x2; pack with swiglu_perm), bias, and
      "bias"    want = x.W + b, integers of magnitude <= 24
      "resid"   resid integers in [-96, 96], gamma in {1/2, 1, 2}: want = resid + gamma (x.W + b) and want_nogamma
      "gelu"    v = x.W + b in {0} u [8, 40] u [-40, -8] by column class (W row and bias zero; bias +24; bias -24).  Column
                0 of every 32-column block is of the positive class (v >= 8 on every row), the last block is all zero.
                want = v, +0 or GELU_NEG_TAIL
      "swiglu"  gate = x.W1 + b1 in {0} u [32, 64] u [-160, -128] by column class, u = x.W2 + b2 integers in [-3, 3]; the
                last block all zero.  want = silu(gate) * u with silu in {+0, gate, -0}: integers or signed zeros
    want is float32 (signed zeros kept); every want is bf16-exact except the GELU tail"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    if kind in ("bias", "resid"):
        w = _sparse_weight(N, K, g)
        b = torch.randint(-8, 9, (N,), generator=g).float()
        acc = (x.double() @ w.double().t() + b.double()).float()
        if kind == "bias":
            return dict(x=x, w=w, bias=b, want=acc)
        resid = torch.randint(-96, 97, (M, N), generator=g).float()
        gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
        return dict(x=x, w=w, bias=b, resid=resid, gamma=gamma, want=resid + gamma * acc, want_nogamma=resid + acc)
    cls = torch.randint(0, 3, (N,), generator=g)  # 0: zero, 1: positive, 2: negative
    cls[::BLOCK] = 1
    cls[-BLOCK:] = 0
    if kind == "gelu":
        w = _sparse_weight(N, K, g) * (cls != 0)[:, None]
        b = torch.tensor([0.0, 24.0, -24.0])[cls]
        v = (x.double() @ w.double().t() + b.double()).float()
        assert bool(((v == 0) | (v.abs() >= 8)).all())
        want = torch.where(v <= -8, torch.full_like(v, GELU_NEG_TAIL), v)
        return dict(x=x, w=w, bias=b, pre=v, want=want)
    if kind == "swiglu":
        w1 = _sparse_weight(N, K, g) * (cls != 0)[:, None]
        b1 = torch.tensor([0.0, 48.0, -144.0])[cls]
        w2 = _sparse_weight(N, K, g, nnz=1) * (cls != 0)[:, None]
        b2 = torch.randint(-2, 3, (N,), generator=g).float() * (cls != 0)
        gate = (x.double() @ w1.double().t() + b1.double()).float()
        u = (x.double() @ w2.double().t() + b2.double()).float()
        assert bool(((gate == 0) | (gate >= 32) | (gate <= -128)).all()) and float(u.abs().max()) <= 3
        s = torch.where(gate >= 32, gate, torch.where(gate == 0, torch.zeros_like(gate), -torch.zeros_like(gate)))
        return dict(x=x, w=torch.cat([w1, w2]), bias=torch.cat([b1, b2]), pre=gate, pre_u=u, want=s * u)
    raise ValueError(kind)


def gelu_exact_case(M: int, N: int, K: int, seed: int = 0):
    return epilogue_case("gelu", M, N, K, seed)


def swiglu_exact_case(M: int, N: int, K: int, seed: int = 0):
    return epilogue_case("swiglu", M, N, K, seed)


def second_weight(N2: int, K2: int, seed: int = 0) -> torch.Tensor:
    """[N2, K2] of -1 / 0 / +1, 2 non-zeros per row: the integer product that follows an MX-out GEMM (the fed operand
    holds integers of magnitude <= 192; the caller asserts that the product is bf16-exact)"""
    return _sparse_weight(N2, K2, torch.Generator().manual_seed(seed), nnz=2)


# ---- model of the GEMM and of its MX-out epilogue -----------------------------------------------------------------
def model_linear_mx(aq, as_flat, wq, ws_flat, bug: str | None = None) -> torch.Tensor:
    """float64 A.W^T of two raw MX tensors (payload bytes, flat scale arrays), reading the scales as the GEMM does.
    Bugs: BUGS_GEMM"""
    M, K = aq.shape
    N = wq.shape[0]
    lay = bug if bug in ("pair_swapped", "rows_pad_as_rows") else None
    if bug == "scales_exchanged":
        # sA and sW swapped: row m of A reads W's array at its own slot (zero-filled where W has fewer rows)
        big = max(mx_rows_pad(M), mx_rows_pad(N))
        sa = torch.zeros(K // 32, big, dtype=torch.uint8)
        sa[:, :mx_rows_pad(N)] = ws_flat.reshape(K // 32, -1)
        sw = torch.zeros(K // 32, big, dtype=torch.uint8)
        sw[:, :mx_rows_pad(M)] = as_flat.reshape(K // 32, -1)
        sa_r = sa[:, mx_scale_slot(torch.arange(M))].t()
        sw_r = sw[:, mx_scale_slot(torch.arange(N))].t()
    else:
        sa_r, sw_r = gather_scales(as_flat, M, K, lay), gather_scales(ws_flat, N, K, lay)
    if bug == "neighbour_scale":
        sa_r = sa_r.reshape(M, -1)[:, torch.arange(K // 32) ^ 1] if K >= 64 else sa_r
    return decode(aq, sa_r) @ decode(wq, sw_r).t()


def model_epilogue_mx(case: dict, kind: str, bug: str | None = None):
    """the MX-out epilogue on a gelu / swiglu epilogue_case: (payload [M, N], flat scales).  Bugs: BUGS_EPI"""
    want, pre = case["want"], case["pre"]
    M, N = want.shape
    if bug == "no_fold" and kind == "swiglu":
        # packed column n (its x1 half) stored at column n instead of (n >> 6) * 32 + (n & 31)
        out = torch.zeros_like(want)
        for blk in range(N // 32):
            if 64 * blk + 32 <= N:
                out[:, 64 * blk:64 * blk + 32] = want[:, 32 * blk:32 * blk + 32]
        want = out
    if bug == "amax_before_act":
        a = pre.abs().reshape(M, N // 32, 32).amax(-1)
        e = mx.scale_exponent(a)
        y = want.reshape(M, N // 32, 32) * torch.ldexp(torch.ones_like(a), -e)[..., None]
        return e4m3_round(y.clamp(-448, 448)).reshape(M, N), place_scales((e + 127).to(torch.uint8))
    return model_quantize(want, bug=bug if bug != "no_fold" else None)


# ---- LayerNorm to MX ----------------------------------------------------------------------------------------------
def ln_mx_case(M: int, D: int, seed: int = 0):
    """dict: x [M, D] (ln_fold_designs.cycled_rows: bf16-exact, exact means, |mean| / sigma up to 192, constant rows),
    gamma powers of two in {1/2, 1, 2, 4}, beta multiples of 1/8 in [-1, 1], ref (float64 LayerNorm), scale (the S of
    the module docstring), const (mask of the constant rows, whose output is exactly beta)"""
    g = torch.Generator().manual_seed(1000 * D + M + seed)
    x = cycled_rows(M, D, seed=seed + D)
    gamma = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (D,), generator=g)]
    beta = torch.randint(-8, 9, (D,), generator=g).float() / 8.0
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    n = (xd - mu) / torch.sqrt(var + eps) * gamma.double()
    return dict(x=x, gamma=gamma, beta=beta, ref=n + beta.double(), scale=n.abs() + beta.double().abs(),
                const=(var.reshape(-1) == 0))


def model_ln(x, gamma, beta, eps: float = EPS, bug: str | None = None) -> torch.Tensor:
    """fp32 model of ln_mx_kernel's arithmetic (csrc/mx.hip): mean = sum * (1 / D), var = sum (x - mean)^2 * (1 / D), rstd = rsqrt(var + eps),
    (x - mean) * rstd * gamma + beta, every step rounded to fp32.  Bugs: BUGS_LN"""
    x = x.float()
    D = x.shape[1]
    s = x.sum(1, keepdim=True)
    inv = torch.tensor(1.0 / D, dtype=torch.float32)
    mean = s * inv  # (the kernel multiplies by the float 1 / D)
    d = x - mean
    ss = (d * d).sum(1, keepdim=True)
    var = ss / (D - 1) if bug == "unbiased" else ss * inv
    e = torch.tensor(eps, dtype=torch.float32)
    rstd = 1.0 / (torch.sqrt(var) + e) if bug == "eps_outside" else 1.0 / torch.sqrt(var + e)
    return d * rstd * gamma.float() + beta.float()


def model_ln_mx(case: dict, bug: str | None = None):
    """(payload, scale bytes [M, D/32]) of the LayerNorm-to-MX model; LayerNorm bugs BUGS_LN, quantiser bugs BUGS_QUANT"""
    o = model_ln(case["x"], case["gamma"], case["beta"], bug=bug if bug in BUGS_LN else None)
    q, flat = model_quantize(o, bug=bug if bug in BUGS_QUANT else None)
    return q, gather_scales(flat, *o.shape)


def ulp32(s: torch.Tensor) -> torch.Tensor:
    s = s.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(s)) - 23)


def measured_noise_ulps(case: dict) -> float:
    """largest |float64 LayerNorm - fp32 model| in fp32 ulps of S, over one case"""
    o = model_ln(case["x"], case["gamma"], case["beta"]).double()
    return float(((o - case["ref"]).abs() / ulp32(case["scale"])).max())


# ---- checks -------------------------------------------------------------------------------------------------------
def _first(bad: torch.Tensor):
    return tuple(bad.nonzero()[0].tolist())


def check_bytes_equal(got_q, got_s, want_q, want_s, what: str = ""):
    """payload [rows, K] and scale bytes [rows, K/32], every byte"""
    got_q, got_s = got_q.cpu(), got_s.cpu()
    bad = got_s != want_s
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} scale bytes differ (first at row {i[0]} block "
                             f"{i[1]}: got {int(got_s[i])}, want {int(want_s[i])})")
    bad = got_q != want_q
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} payload bytes differ (first at {list(i)}: got "
                             f"{int(got_q[i]):#04x}, want {int(want_q[i]):#04x})")


def check_mx_bytes(got_q, got_s, ref64, noise, what: str = "", cap: float = MAX_EXCLUDED_FRAC) -> int:
    """got payload [M, D] / scale bytes [M, D/32] == the oracle quantiser of the float64 reference, every byte, except
      an element whose scaled reference lies within its (scaled) `noise` of an e4m3 rounding midpoint,
      a block (its 32 elements and its scale) whose maximum / 448 lies within the block's largest noise / 448 of a
      power of two.
    noise [M, D] is absolute (NOISE_ULPS * ulp32(S)).  Returns the number of excluded elements, at most cap * M * D"""
    got_q, got_s = got_q.cpu(), got_s.cpu()
    ref = ref64.double().cpu()
    M, D = ref.shape
    nb = D // BLOCK
    want_q, want_s = encode(ref.float())
    rb = ref.reshape(M, nb, BLOCK)
    nz = noise.double().reshape(M, nb, BLOCK)
    t = rb.abs().amax(-1) / 448.0
    p2 = torch.exp2(torch.round(torch.log2(t.clamp_min(2.0 ** -140))))
    blk_excl = (t - p2).abs() < nz.amax(-1) / 448.0
    e = want_s.to(torch.int32) - 127
    sc = torch.ldexp(torch.ones(M, nb, dtype=torch.float64), -e)[..., None]
    a, ny = (rb * sc).abs(), nz * sc
    ex = torch.floor(torch.log2(a)).clamp(min=-6.0)
    ex = torch.where(a == 0, torch.full_like(ex, -6.0), ex)
    step = torch.exp2(ex - 3)
    f = a / step
    el_excl = ((f - torch.floor(f) - 0.5).abs() * step < ny) | blk_excl[..., None]
    el_excl = el_excl.reshape(M, D)
    bad_s = (got_s != want_s) & ~blk_excl
    if bad_s.any():
        i = _first(bad_s)
        raise AssertionError(f"{what}: {int(bad_s.sum())} of {bad_s.numel()} scale bytes differ from the oracle's (first "
                             f"at row {i[0]} block {i[1]}: got {int(got_s[i])}, want {int(want_s[i])})")
    bad = (got_q != want_q) & ~el_excl
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} payload bytes differ from the oracle's (first "
                             f"at {list(i)}: got {int(got_q[i]):#04x}, want {int(want_q[i]):#04x}, ref {ref[i].item()!r})")
    n = int(el_excl.sum())
    assert n <= cap * M * D, f"{what}: {n} of {M * D} elements within the noise of a rounding boundary (cap {cap:g})"
    return n


def ln_noise(case: dict) -> torch.Tensor:
    """[M, D] absolute noise of a LayerNorm case: NOISE_ULPS fp32 ulps of S; none on the constant rows, where
    x - mean = 0 and the output is beta exactly"""
    n = NOISE_ULPS * ulp32(case["scale"])
    n[case["const"]] = 0.0
    return n


def check_exact_bf16_bits(got: torch.Tensor, want: torch.Tensor, what: str = ""):
    """bf16 output == bf16(want) bit for bit (signed zeros included)"""
    g = got.cpu().contiguous().view(torch.int16)
    w = want.float().to(torch.bfloat16).contiguous().view(torch.int16)
    bad = g != w
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (first at {list(i)}: got "
                             f"{got.cpu().float()[i].item()!r}, want {want[i].item()!r})")

