"""Designed attention inputs whose bf16 output is known exactly, the checks that go with them, and a torch model of
the attention kernels' arithmetic.

TEST INFRASTRUCTURE ONLY (never imported by the product package).

tests/test_attention_exact_gpu.py runs the constructions through every attention kernel; tests/test_attention_gates_cpu.py
runs them through `model_attention` with and without injected bugs, to show that each check rejects the bugs it is
meant to catch.  Tensors are [B, N, H, dh] float32 holding bf16 values unless stated otherwise.

  uniform_case      Q = 0: every score is 0, P = 1, the output is the plain mean of the valid V rows, built to be
                    exactly c[b, h] (one dropped, extra or duplicated key moves it)
  onehot_case       Q_i = a K_pi(i) for +-1 codes K: query i picks key pi(i) with a softmax gap >= GAP_NATS, the output
                    is exactly V[pi(i)] (a key routed from the wrong head or the wrong place moves it)
  relpos_spike_case Q = a e0, K = 0, one spike per rel-pos table: the bias alone picks key (qh - dh, qw - dw)
  beta              <got - ref, ref> / <ref, ref>: a kernel that is right up to rounding has |beta| ~ 1e-5 on random
                    data; a softmax temperature, P rounding or denominator bug biases every output the same way
"""
from __future__ import annotations

import math

import torch

GAP_NATS = 24.0     # softmax gap of the one-hot constructions: the other keys' weights sum to < 1e-7 at 4096 keys
BETA_GATE = 3e-4    # |beta| bound of the random-data tests
BETA_MIN_N = 30000  # ... applied from this many outputs on
LOG2E = 1.44269504088896341


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): the bug the RNE convert must not have."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def full_lens(B: int, N: int) -> torch.Tensor:
    return torch.full((B,), N, dtype=torch.int64)


def valid_rows(lens: torch.Tensor, N: int) -> torch.Tensor:
    """[B, N] bool: row j of sequence b is < its length"""
    return torch.arange(N)[None, :] < lens.cpu()[:, None]


def pack_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """[B, N, H, dh] x 3 -> the packed [B*N, 3*H*dh] bf16 activation (columns [q | k | v], each [H, dh])"""
    B, N, H, dh = q.shape
    return torch.cat([t.reshape(B, N, H * dh) for t in (q, k, v)], dim=-1).reshape(B * N, 3 * H * dh).to(torch.bfloat16)


def unpack_qkv(qkv: torch.Tensor, B: int, N: int, H: int, dh: int):
    q, k, v = qkv.float().reshape(B, N, 3, H, dh).unbind(2)
    return q, k, v


def fill_padding(qkv: torch.Tensor, lens: torch.Tensor, N: int, value: float) -> torch.Tensor:
    """a copy of the packed activation with every column of every row past its sequence's length set to `value`"""
    out = qkv.clone()
    pad = ~valid_rows(lens, N).reshape(-1).to(qkv.device)
    out[pad] = value
    return out


def check_lens(B: int, N: int, lens):
    lens = full_lens(B, N) if lens is None else torch.as_tensor(lens, dtype=torch.int64).cpu()
    assert lens.shape == (B,) and int(lens.min()) >= 1 and int(lens.max()) <= N
    return lens


# ---- uniform attention ------------------------------------------------------------------------------------------
def zero_sum_deviations(L: int, g: torch.Generator) -> torch.Tensor:
    """L integers, none 0 (L > 1), summing to 0, |d| <= 14: pairs (+t, -t) and, for odd L, one (+2t, -t, -t);
    in a random order.  L = 1: [0]."""
    if L == 1:
        return torch.zeros(1)
    n_pairs = L // 2 if L % 2 == 0 else (L - 3) // 2
    t = torch.randint(1, 8, (n_pairs,), generator=g).float()
    parts = [t, -t]
    if L % 2:
        t3 = torch.randint(1, 8, (1,), generator=g).float()
        parts.append(torch.cat([2 * t3, -t3, -t3]))
    d = torch.cat(parts)
    return d[torch.randperm(L, generator=g)]


def uniform_case(B: int, N: int, H: int, dh: int, lens=None, seed: int = 0):
    """Q = 0, so every score is exactly 0 and P = 1 whatever K holds (random, large).  V[b, j, h, col] =
    c[b, h, col] + d[b, h, j] with integer deviations d != 0 that sum to zero over the valid keys, everything in units
    of 2^e[b, h] and below 256 units: V is bf16, every partial sum of P.V and of the row sum is exact in fp32, and
    len * c * fl(1 / len) rounds back to c in bf16 -- the output of every valid row is exactly c, whatever the
    reciprocal's last ulp.  c = 0 in the even columns (there a dropped, extra or duplicated key gives a non-zero value)
    and distinct per (b, h, col) in the odd ones (routing).  Padding rows: Q = 0, K random, V = 2^12 units."""
    lens = check_lens(B, N, lens)
    g = torch.Generator().manual_seed(seed)
    half = dh // 2
    # odd columns: c = m 2^e with |m| in [128, 241] (one binade: distinct m and e give distinct c), both signs -- 228
    # values per exponent; |m + d| <= 255
    per_e = 228 // half                 # (b, h) pairs per exponent
    bh = torch.arange(B * H)
    e = (bh // per_e - 24).float()
    assert int(e.max()) < 100, "too many (b, h) pairs for distinct c"
    unit = torch.pow(2.0, e)            # [BH]
    slot = bh % per_e
    vidx = slot[:, None] * half + torch.arange(half)[None, :]           # [BH, half] in [0, 228)
    m = (128 + vidx // 2).float() * (1 - 2 * (vidx % 2)).float()
    c = torch.zeros(B * H, dh)
    c[:, 1::2] = m * unit[:, None]
    d = torch.zeros(B * H, N)
    for i in range(B * H):
        L = int(lens[i // H])
        d[i, :L] = zero_sum_deviations(L, g) * unit[i]
    c4 = c.reshape(B, H, dh)
    v = c4[:, None, :, :] + d.reshape(B, H, N).permute(0, 2, 1)[..., None]  # [B, N, H, dh]
    pad = ~valid_rows(lens, N)
    v[pad] = (4096.0 * unit.reshape(B, H))[:, None, :, None].expand(B, N, H, dh)[pad]
    k = bf16_round(torch.randn(B, N, H, dh, generator=g) * 300.0)
    q = torch.zeros(B, N, H, dh)
    assert torch.equal(bf16_round(v), v)
    expected = c4[:, None, :, :].expand(B, N, H, dh).clone()
    return dict(q=q, k=k, v=v, expected=expected, lens=lens, c=c4, d=d.reshape(B, H, N), unit=unit.reshape(B, H))


# ---- one-hot permutation ----------------------------------------------------------------------------------------
def _rand_v(shape, g):
    """+-[1, 2) on the bf16 grid"""
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (1 + torch.randint(0, 128, shape, generator=g).float() / 128)


def code_gap(k: torch.Tensor, lens: torch.Tensor, device=None) -> torch.Tensor:
    """per (b, h): dh - max over valid keys t != j of K_t . K_j, for +-1 codes K (an integer, 2 x the smallest
    Hamming distance to another valid key).  Computed in float64 on `device`."""
    B, N, H, dh = k.shape
    kt = k.to(device or k.device, torch.float64).permute(0, 2, 1, 3)  # [B, H, N, dh]
    gm = kt @ kt.transpose(-1, -2)
    valid = valid_rows(lens, N).to(gm.device)
    bad = ~(valid[:, None, :, None] & valid[:, None, None, :]) | torch.eye(N, dtype=torch.bool, device=gm.device)
    gm = gm.masked_fill(bad, -math.inf)
    other = gm.amax(dim=(-1, -2))
    other = torch.where(torch.isfinite(other), other, torch.full_like(other, -dh))  # one valid key: no other
    return (dh - other).cpu()


def onehot_case(B: int, N: int, H: int, dh: int, lens=None, seed: int = 0, device=None):
    """K rows are +-1 codes; Q_i = a K_pi(i) with pi a permutation of the valid keys, different per (b, h); a is the
    smallest power of two that puts the target's score >= GAP_NATS nats (after dh^-1/2) above every other valid
    key's.  V in +-[1, 2).  Expected output: V[pi(i)] exactly (the other keys' weights sum to < 1e-7 of the target's
    and rounding the target's P ~ 1 to bf16 gives 1).  Padding rows are adversarial: K = 2 x the code of a valid
    key (a leaked key would win), V = 64, Q = a x a code.  `device`: where the gap is computed (N^2 dh per (b, h))."""
    lens = check_lens(B, N, lens)
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 2, (B, N, H, dh), generator=g).float() * 2 - 1
    v = _rand_v((B, N, H, dh), g)
    gap = code_gap(k, lens, device)
    min_gap = float(gap.min())
    assert min_gap > 0, "two valid keys share a code"
    a = 2.0 ** math.ceil(math.log2(GAP_NATS * math.sqrt(dh) / min_gap))
    q = torch.empty(B, N, H, dh)
    expected = torch.empty(B, N, H, dh)
    for b in range(B):
        L = int(lens[b])
        for h in range(H):
            pi = torch.randperm(L, generator=g)
            q[b, :L, h] = a * k[b, pi, h]
            expected[b, :L, h] = v[b, pi, h]
            pad = torch.arange(L, N) % L
            q[b, L:, h] = a * k[b, pad, h]
            expected[b, L:, h] = float("nan")
            k[b, L:, h] = 2 * k[b, pad, h]
            v[b, L:, h] = 64.0
    return dict(q=q, k=k, v=v, expected=expected, lens=lens, a=a, gap_nats=a * min_gap / math.sqrt(dh), gaps=gap)


# ---- relative position bias -------------------------------------------------------------------------------------
def relpos_spike_case(B: int, S: int, H: int, delta, seed: int = 0):
    """SAM attention over S x S grids: Q = 32 e0, K = 0, rel_pos_h[:, 0] and rel_pos_w[:, 0] zero but for a 1 at
    relative offsets delta = (dh, dw).  Logit of key (kh, kw) for query (qh, qw): 32 [qh - kh == dh] + 32 [qw - kw == dw]
    (q . Rh[qh - kh + S - 1] in the kernel's index convention).  Where (qh - dh, qw - dw) is inside the grid that key
    leads every other by 32 nats: the output is exactly its V.  Returns qkv parts, the two tables and, per query, the
    target key or -1."""
    g = torch.Generator().manual_seed(seed)
    n = S * S
    q = torch.zeros(B, n, H, 64)
    q[..., 0] = 32.0
    k = torch.zeros(B, n, H, 64)
    v = _rand_v((B, n, H, 64), g)
    rel_h = torch.zeros(2 * S - 1, 64)
    rel_w = torch.zeros(2 * S - 1, 64)
    rel_h[delta[0] + S - 1, 0] = 1.0
    rel_w[delta[1] + S - 1, 0] = 1.0
    qh, qw = torch.arange(n) // S, torch.arange(n) % S
    th, tw = qh - delta[0], qw - delta[1]
    inside = (th >= 0) & (th < S) & (tw >= 0) & (tw < S)
    target = torch.where(inside, th * S + tw, torch.full_like(th, -1))
    return dict(q=q, k=k, v=v, rel_h=rel_h, rel_w=rel_w, target=target)


def relpos_onehot_case(B: int, S: int, H: int, seed: int = 0, device=None):
    """onehot_case over an S x S grid with zero rel-pos tables (the bias adds exactly 0)"""
    c = onehot_case(B, S * S, H, 64, seed=seed, device=device)
    c["rel_h"] = torch.zeros(2 * S - 1, 64)
    c["rel_w"] = torch.zeros(2 * S - 1, 64)
    return c


# ---- references and checks --------------------------------------------------------------------------------------
def ref_attention(q, k, v, lens=None, device=None) -> torch.Tensor:
    """softmax(q k^T dh^-1/2) v over the valid keys, float64, [B, N, H, dh]"""
    B, N, H, dh = q.shape
    lens = check_lens(B, N, lens)
    dev = device or q.device
    qt, kt, vt = (t.to(dev, torch.float64).permute(0, 2, 1, 3) for t in (q, k, v))
    s = (qt @ kt.transpose(-1, -2)) / math.sqrt(dh)
    keep = valid_rows(lens, N).to(dev)[:, None, None, :]
    s = s.masked_fill(~keep, -math.inf)
    vt = vt.masked_fill(~keep.transpose(-1, -2), 0.0)
    return (torch.softmax(s, dim=-1) @ vt).permute(0, 2, 1, 3)


def beta(got: torch.Tensor, ref: torch.Tensor) -> float:
    """<got - ref, ref> / <ref, ref> in float64: the share of the reference the error points along"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1).to(got.device)
    return float(((got - ref) @ ref) / (ref @ ref))


def check_unbiased(got: torch.Tensor, ref: torch.Tensor, what: str = "", gate: float = BETA_GATE) -> float | None:
    """assert |beta| <= gate where there are at least BETA_MIN_N outputs; returns beta (None below that size)"""
    if got.numel() < BETA_MIN_N:
        return None
    b = beta(got, ref)
    assert abs(b) <= gate, f"{what}: beta = {b:.3e} (|beta| > {gate:g}: the outputs are biased along the reference)"
    return b


def check_exact(got: torch.Tensor, expected: torch.Tensor, rows: torch.Tensor | None = None, what: str = ""):
    """bitwise equality of bf16 outputs [B, N, H, dh] on the rows selected by `rows` ([B, N] bool, default all)"""
    got, expected = got.float().cpu(), expected.float().cpu()
    if rows is not None:
        got, expected = got[rows], expected[rows]
    bad = got.view(torch.int32) != expected.view(torch.int32)
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs not bit-exact; first at {i}: got "
                             f"{got[tuple(i)].item():.8g} want {expected[tuple(i)].item():.8g}")


# ---- a model of the kernels' arithmetic -------------------------------------------------------------------------
BUGS = ("drop_key", "extra_zero_key", "dup_last_key", "trunc_p", "temperature", "cross_head_k", "len_off_by_one",
        "nan_padding")


def model_attention(q, k, v, lens=None, bug: str | None = None) -> torch.Tensor:
    """What the attention kernels compute, in torch: bf16 q / k / v, fp32 scores, P = exp2(s dh^-1/2 log2e - max),
    P rounded to bf16 (RNE) for P.V while the row sum adds the fp32 P, fp32 accumulation, bf16 output of
    O * (1 / l).  Keys past a sequence's length are masked; the V rows staged for them repeat its last valid row.
    `bug` injects one of BUGS:
      drop_key        the middle valid key is left out       extra_zero_key  one more key, score 0 and V 0
      dup_last_key    the last valid key counts twice        trunc_p         P truncated to bf16, not rounded
      temperature     the exp2 scale is 0.2 % too large      cross_head_k    head h reads the K of head h + 1
      len_off_by_one  one key past the length is valid       nan_padding     padding V rows staged as they are
    Returns [B, N, H, dh] float32 (bf16 values)."""
    assert bug is None or bug in BUGS, bug
    B, N, H, dh = q.shape
    lens = check_lens(B, N, lens)
    sc = float(torch.tensor(dh ** -0.5 * LOG2E, dtype=torch.float32))
    if bug == "temperature":
        sc *= 1.002
    if bug == "cross_head_k":
        k = k.roll(-1, dims=2)
    eff = lens + 1 if bug == "len_off_by_one" else lens
    eff = eff.clamp(max=N)
    qt, kt, vt = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))  # [B, H, N, dh]
    keep = valid_rows(eff, N)                                         # [B, N]
    if bug == "drop_key":
        keep[torch.arange(B), eff // 2] = False
    if bug != "nan_padding":  # the staged V rows past the length repeat the last valid row
        idx = torch.minimum(torch.arange(N)[None, :], eff[:, None] - 1)  # [B, N]
        vt = torch.gather(vt, 2, idx[:, None, :, None].expand(B, H, N, dh))
    s = qt @ kt.transpose(-1, -2)
    s = s.masked_fill(~keep[:, None, None, :], -math.inf)
    if bug == "dup_last_key":
        last = eff - 1
        s = torch.cat([s, s[torch.arange(B), :, :, last][:, :, :, None]], dim=-1)
        vt = torch.cat([vt, vt[torch.arange(B), :, last][:, :, None, :]], dim=2)
    if bug == "extra_zero_key":
        s = torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)
        vt = torch.cat([vt, torch.zeros_like(vt[:, :, :1])], dim=2)
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp2(s * sc - m * sc)
    l = p.sum(dim=-1, keepdim=True)
    pb = bf16_trunc(p) if bug == "trunc_p" else bf16_round(p)
    o = pb @ vt
    return bf16_round(o * (1.0 / l)).permute(0, 2, 1, 3)
