"""Designed inputs for the folded LayerNorm, the checks that go with them, and a torch model of its arithmetic.

TEST INFRASTRUCTURE ONLY (never imported by the product package).

The fold (csrc/gemm_epi.h, gemm_kernels.h, vdr_api.hip fold_ln_host) runs in four parts: the residual GEMM writes fp32
(sum, sumsq) partials of its stored bf16 rows per 64-column group; a finaliser turns them into (mean, rstd) in double;
the host folds gamma into the weight (W' = bf16(gamma W), colsum = sum W', tbias = sum beta W + b); the consumer GEMM
computes rstd (x.W'^T - mean colsum) + tbias.  tests/test_ln_fold_gpu.py runs the constructions below through the
kernels; tests/test_ln_fold_gates_cpu.py runs them through `model_*` with and without injected bugs, to show that each
check rejects the bugs it is meant to catch.

  designed_rows    x = mu + sigma s with s a zero-sum pattern of -1 / 0 / +1 (variance 1/2 or 2/3): every x is
                   bf16-exact, every partial an exact fp32 sum, the exact mean is mu
  designed_weights gamma powers of two (and 1 + 2^-9, which rounds away in bf16), W small integers, beta dyadic, b
                   small: W', colsum and tbias are exact, and so is the GEMM's accumulator x.W'^T
  check_exact_bf16 got == bf16(ref) except where the float64 reference lies within TIE_REL * fold_noise_scale of a
                   bf16 rounding tie: the epilogue forms rstd acc - rstd mean colsum in fp32, so its noise is a few
                   ulps of rstd |acc| (growing with |mean| / sigma), not of the output.  The count of excluded
                   elements is returned and bounded
"""
from __future__ import annotations

from fractions import Fraction

import torch

TIE_REL = 2.0 ** -23  # |ref - tie| below this times fold_noise_scale (~2 rstd |acc|: 4 fp32 ulps of it) may round either way
EPS = 1e-6
BUGS_STATS = ("unbiased", "eps_outside", "float_inv_d", "prerounding", "drop_last", "double_last", "neighbour")
BUGS_FOLD = ("colsum_unrounded", "tbias_no_beta", "swiglu_x1_colsum")


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.bfloat16).float()


# ---- designed inputs ----------------------------------------------------------------------------------------------
def zero_sum_patterns(M: int, D: int, seed: int) -> torch.Tensor:
    """[M, D] rows of -1 / 0 / +1 with sum 0: a shuffled quarter +1, quarter -1 (variance 1/2), or on every other row
    (D % 3 == 0) a third each (variance 2/3).  The variances are not squares, so rstd is irrational and the designed
    outputs do not land on bf16 rounding ties"""
    g = torch.Generator().manual_seed(seed)
    base1 = torch.zeros(D)
    base1[: D // 4] = 1.0
    base1[D // 4: D // 2] = -1.0
    base2 = torch.zeros(D)
    base2[: D // 3] = 1.0
    base2[D // 3: 2 * (D // 3)] = -1.0
    rows = []
    for r in range(M):
        base = base2 if (r % 2 == 1 and D % 3 == 0) else base1
        rows.append(base[torch.randperm(D, generator=g)])
    return torch.stack(rows)


def designed_rows(M: int, D: int, mu, sigma, seed: int = 0) -> torch.Tensor:
    """x = mu + sigma s, fp32 holding bf16-exact values; mu / sigma scalars or [M] tensors (sigma 0: constant rows)"""
    s = zero_sum_patterns(M, D, seed)
    mu = torch.as_tensor(mu, dtype=torch.float64).reshape(-1, 1).expand(M, 1)
    sigma = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1, 1).expand(M, 1)
    x = mu + sigma * s.double()
    assert torch.equal(bf16_round(x).double(), x), "designed rows must be bf16-exact"
    return x.float()


def designed_weights(N: int, K: int, seed: int = 0):
    """(W, b, gamma, beta) fp32: gamma in {1/2, 1, 2, 1 + 2^-9}, W integers in [-3, 3], beta multiples of 1/8, b
    integers.  gamma = 1 + 2^-9 is not dyadic-short: gamma W rounds to W in bf16, so a colsum of the unrounded product
    differs from that of the stored weight"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    gamma = torch.tensor([0.5, 1.0, 2.0, 1.0 + 2.0 ** -9])[torch.randint(0, 4, (K,), generator=g)]
    beta = torch.randint(-8, 9, (K,), generator=g).float() / 8.0
    b = torch.randint(-4, 5, (N,), generator=g).float()
    return W, b, gamma, beta


def swiglu_perm(F2: int) -> torch.Tensor:
    """packed row -> source row of mlp.w12 (the layout of ops.pack_w12)"""
    idx = torch.arange(F2)
    blk, t = idx // 64, idx % 64
    return torch.where(t < 32, blk * 32 + t, F2 // 2 + blk * 32 + (t - 32))


# (mean, sigma) of the designed rows, cycled over M: |mean| / sigma in {0, 16, 64, 192}, small sigma (eps matters:
# var ~ 1.2e-4), and constant rows (sigma 0: the output is exactly bf16(tbias))
ROW_CLASSES = ((0.0, 1.0), (16.0, 1.0), (64.0, 1.0), (192.0, 1.0), (-192.0, 1.0), (1.0, 2.0 ** -6), (0.0, 4.0),
               (-64.0, 2.0), (3.0, 0.0), (96.0, 0.5))


def cycled_rows(M: int, D: int, seed: int = 0, classes=ROW_CLASSES) -> torch.Tensor:
    mu = torch.tensor([classes[r % len(classes)][0] for r in range(M)])
    sigma = torch.tensor([classes[r % len(classes)][1] for r in range(M)])
    return designed_rows(M, D, mu, sigma, seed)


def integer_producer_case(M: int, N: int, K: int, seed: int = 0, layerscale: bool = False):
    """(x, W, b, resid, gamma) whose residual output resid + gamma (x W^T + b) is an integer of magnitude <= 144 (a
    half-integer below 128 where gamma = 1/2): bf16-exact, so every (sum, sumsq) partial is an exact fp32 sum"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    W = torch.zeros(N, K)
    W[:, :16] = torch.randint(-1, 2, (N, 16), generator=g).float()  # |x W^T| <= 16
    b = torch.randint(-8, 9, (N,), generator=g).float()
    resid = torch.randint(-96, 97, (M, N), generator=g).float()  # |y| <= 144; half-integers (gamma 1/2) only below 128
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)] if layerscale else None
    return x, W, b, resid, gamma


def model_producer(x, W, b, resid, gamma=None) -> torch.Tensor:
    """pre-rounding fp32 output of the residual epilogue"""
    y = x.double() @ W.double().t() + b.double()
    if gamma is not None:
        y = y * gamma.double()
    return (y + resid.double()).float()


def ref_fold(x, Wf, W, b, beta, eps: float = EPS) -> torch.Tensor:
    """float64 (x - mean) / sqrt(var + eps) . Wf^T + beta . W^T + b: the fold's exact target for the stored folded weight
    Wf (= gamma W when gamma W is bf16-exact)"""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    return ((xd - mu) / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))) @ Wf.double().t() + \
        (beta.double() @ W.double().t() + b.double())


# ---- model of the arithmetic --------------------------------------------------------------------------------------
def model_partials(y: torch.Tensor, bug: str | None = None) -> torch.Tensor:
    """(sum, sumsq) per 64-column group of the STORED bf16 rows: [D/64, M, 2] fp32.  y holds the pre-rounding values
    (fp32); bug "prerounding": statistics of those instead of the bf16 copy"""
    v = y.double() if bug == "prerounding" else bf16_round(y).double()
    M, D = v.shape
    g = v.reshape(M, D // 64, 64)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], -1).permute(1, 0, 2).float().contiguous()


def _fma_exact(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # correctly rounded a * b + c


def model_finalize(part: torch.Tensor, eps: float = EPS, bug: str | None = None) -> torch.Tensor:
    """[G, M, 2] partials -> [M, 2] (mean, rstd) fp32: the finalisers' formula (csrc/vdr_dev.h ln_mean_rstd) in float64,
    the groups summed in order, var = fma(-mean, mean, s2 / D)"""
    G, M, _ = part.shape
    p = part.double()
    if bug == "drop_last":
        p = p[:-1]
    elif bug == "double_last":
        p = torch.cat([p, p[-1:]], 0)
    D = 64 * G
    out = torch.empty(M, 2, dtype=torch.float64)
    eps_d = float(torch.tensor(eps, dtype=torch.float32))
    inv_f = float(torch.tensor(1.0 / D, dtype=torch.float32))
    for r in range(M):
        s1 = s2 = 0.0
        for gi in range(p.shape[0]):
            s1 += float(p[gi, r, 0])
            s2 += float(p[gi, r, 1])
        if bug == "float_inv_d":  # the float 1/D the finalisers shipped with
            mean = s1 * inv_f
            var = _fma_exact(-mean, mean, s2 * inv_f)
        elif bug == "unbiased":
            mean = s1 / D
            var = (s2 - D * mean * mean) / (D - 1)
        else:
            mean = s1 / D
            var = _fma_exact(-mean, mean, s2 / D)
        var = max(var, 0.0)
        rstd = 1.0 / (var ** 0.5 + eps_d) if bug == "eps_outside" else 1.0 / (var + eps_d) ** 0.5
        out[r, 0], out[r, 1] = mean, rstd
    out = out.float()
    if bug == "neighbour":
        out = torch.roll(out, -1, 0)
    return out


def model_fold(W, b, gamma, beta, swiglu: bool = False, bug: str | None = None):
    """(Wf bf16-valued fp32 [N, K], colsum fp32 [N], tbias fp32 [N]), rows in gate-pair order when swiglu"""
    if swiglu:
        P = swiglu_perm(W.shape[0])
        W, b = W[P], b[P]
    gw = gamma.float() * W.float()  # fp32 product, then RNE to bf16
    Wf = bf16_round(gw)
    colsum = (gw.double() if bug == "colsum_unrounded" else Wf.double()).sum(1).float()
    tb = ((0.0 if bug == "tbias_no_beta" else beta.double()) * W.double()).sum(1) + b.double()
    return Wf, colsum, tb.float()


def model_consumer(x, Wf, colsum, tbias, stats, epilogue: str = "bias", bug: str | None = None) -> torch.Tensor:
    """the consumer GEMM: acc = x.Wf^T (exact on the designed data), rs (acc - mu colsum) + tbias in fp32, then the
    activation; bf16 out.  epilogue "bias" | "gelu" | "swiglu" (columns in gate-pair order)"""
    acc = (x.double() @ Wf.double().t()).float()
    mu, rs = stats[:, :1], stats[:, 1:]
    cs = colsum.clone()
    if bug == "swiglu_x1_colsum":  # the x2 half of every 64-column block reads the colsum of the x1 half
        c = cs.view(-1, 64)
        c[:, 32:] = c[:, :32]
    v = (rs.double() * (acc.double() - mu.double() * cs.double()).float().double()).float() + tbias
    if epilogue == "gelu":
        v = torch.nn.functional.gelu(v.double()).float()
    elif epilogue == "swiglu":
        v = v.view(v.shape[0], -1, 2, 32)
        a, g2 = v[:, :, 0], v[:, :, 1]
        v = (torch.nn.functional.silu(a.double()) * g2.double()).float().reshape(v.shape[0], -1)
    return bf16_round(v)


def ref_consumer(x, W, b, gamma, beta, eps: float = EPS, epilogue: str = "bias") -> torch.Tensor:
    """float64 F.linear(F.layer_norm(x)) (+ activation); swiglu: [M, F] in PyTorch order (x1 | x2 split)"""
    xd = x.double()
    h = torch.nn.functional.layer_norm(xd, (xd.shape[1],), gamma.double(), beta.double(), eps)
    y = h @ W.double().t() + b.double()
    if epilogue == "gelu":
        return torch.nn.functional.gelu(y)
    if epilogue == "swiglu":
        F = y.shape[1] // 2
        return torch.nn.functional.silu(y[:, :F]) * y[:, F:]
    return y


# ---- checks -------------------------------------------------------------------------------------------------------
def fold_noise_scale(x, Wf, colsum, tbias) -> torch.Tensor:
    """[M, N] magnitude the consumer's fp32 epilogue rounds at: the kernels apply the statistics as rstd acc - rstd mean
    colsum + tbias (csrc/gemm_epi.h), so their rounding noise is a few ulps of rstd |acc| -- which grows with |mean| /
    sigma (the fold's inherent cancellation), not of the output"""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))
    acc = xd @ Wf.double().t()
    return rs * (acc.abs() + (mu * colsum.double()).abs()) + tbias.double().abs()


def near_tie(ref: torch.Tensor, scale: torch.Tensor | None = None) -> torch.Tensor:
    """elements whose float64 reference lies within TIE_REL * scale (default |ref|) of a bf16 rounding tie (the midpoint
    between bf16 neighbours)"""
    r = ref.double()
    scale = r.abs() if scale is None else scale.double()
    lo = r.float().to(torch.bfloat16).float().double()
    ulp = torch.where(r.abs() > 0, 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(1e-38))) - 7), torch.zeros_like(r))
    dist = torch.minimum((r - (lo + ulp / 2)).abs(), (r - (lo - ulp / 2)).abs())
    # (an exact tie too: the epilogue's noise decides which way it goes; 1e-10: float64 dust of an exact 0)
    return dist <= TIE_REL * scale + 1e-10


def check_exact_bf16(got: torch.Tensor, ref: torch.Tensor, what: str = "", scale: torch.Tensor | None = None,
                     max_excluded_frac: float = 0.01) -> int:
    """got (bf16) == bf16(ref) wherever ref is not within TIE_REL * scale of a tie; returns the number of excluded
    elements"""
    got = got.float().cpu()
    ref = ref.double().cpu()
    want = ref.float().to(torch.bfloat16).float()
    excl = near_tie(ref, None if scale is None else scale.cpu())
    bad = (got.view(torch.int32) != want.view(torch.int32)) & ~excl
    assert not torch.isnan(got[~excl]).any(), f"{what}: NaN in the output"
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from bf16(ref) "
                             f"(first at {i}: got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}, "
                             f"ref {ref[tuple(i)].item()!r})")
    n = int(excl.sum())
    assert n <= max_excluded_frac * got.numel(), f"{what}: {n} elements within the tie bound"
    return n


def check_stats_bitwise(got: torch.Tensor, want: torch.Tensor, what: str = ""):
    got, want = got.float().cpu().contiguous(), want.float().cpu().contiguous()
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bad.any():
        r = bad.any(1).nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.any(1).sum())} of {got.shape[0]} rows' (mean, rstd) differ "
                             f"(first row {r}: got {got[r].tolist()}, want {want[r].tolist()})")


def check_partials_of(part: torch.Tensor, y_bf16: torch.Tensor, what: str = ""):
    """part [G, M, 2] against the float64 sums of the STORED bf16 rows, at fp32 summation accuracy (64 terms): a
    producer that sums its pre-rounding values is off by ~2^-9 of a term"""
    want = model_partials(y_bf16).double()
    y = y_bf16.double()
    M, D = y.shape
    a = y.abs().reshape(M, D // 64, 64)
    scale = torch.stack([a.sum(-1), (a * a).sum(-1)], -1).permute(1, 0, 2)
    err = (part.double().cpu() - want).abs() - 64 * 2.0 ** -24 * scale
    assert (err <= 0).all(), f"{what}: partials are not those of the stored bf16 rows (max excess {err.max().item():.3e})"


def check_close(got: torch.Tensor, ref: torch.Tensor, rtol: float, atol, what: str = ""):
    got, ref = got.double().cpu(), ref.double().cpu()
    atol = atol.double().cpu() if torch.is_tensor(atol) else atol
    err = (got - ref).abs() - (atol + rtol * ref.abs())
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert (err <= 0).all(), f"{what}: max excess {err.max().item():.3e}"
