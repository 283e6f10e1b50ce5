"""Restatements of vdr_op_upsample_guided (include/vdr.h) for the tests.

upsample_ref      float64 brute force of the definition: per pixel, per window position.  The exponent t of a weight is emulated
                  step by step in numpy float32 (the definition's own roundings, so the `t < -64` decision is the kernel's), the
                  exponential is taken in float64, the weight is split into its two bf16 halves as the definition says, the sums
                  and the division are float64 and the result is rounded once to fp32 and once to the output type.
all_ones_ref      an independent restatement of the all-weights-one case (cs = cr = 0, no confidences): the mean over the in-grid
                  window is avg_pool2d(2r + 1, stride 1, padding r, count_include_pad=False) of the low-resolution map, gathered
                  by nearest_patch.
bound             the entry-wise bound of |kernel - upsample_ref| for random inputs, derived below.
nearest_patch     the i0 rule in integers (the tests compare vdr.upsample.nearest_patch with a brute-force arg-min).

The bound, term by term, relative to S = sum_q w|F| / Z (the weighted mean of |F| over the window; |out| <= S), u = 2^-24:
  weight     the exponent t is at most three fp32 roundings away from its exact value (the product with cs, the product with cr,
             their sum; the squares and the sums under them are counted into the same three since |ts|, |tr| <= |t|), each
             u |t|, and exp turns an absolute error of t into a relative one of w: 3 u |t|max.  The exponential itself: expf of the
             device math library, documented maximum error 1 ulp (HIP math API reference, "expf: 1 ULP"), 2^-23 relative.  The
             product with the confidence: u.  e_w = 3 u |t|max + 2^-23 + u.  It enters the numerator (e_w S) and Z (e_w |out|):
             2 e_w S.
  split      what w_hi + w_lo leaves of w: 2^-16 S (the restatement splits too; the term covers weights that differ in their
             last fp32 bits and therefore in their halves).
  MFMA       K products accumulated in fp32, K = 2 * 16 * ceil((2r+1)^2 / 16) (hi and lo of every slot of the staged step):
             K u S.
  Z          (2r+1)^2 fp32 additions: (2r+1)^2 u S.
  division   u S.
  rounding   to the output type, measured against the UNROUNDED float64 result (rounding both sides would double the term):
             half an ulp of the output format in the entry's own binade, 2^(e - 24) for fp32 and 2^(e - 8) for bf16 (8
             significant bits) with 2^e <= |ref| < 2^(e+1): between 2^-9 |ref| at the top of a binade and 2^-8 |ref| at its
             bottom for bf16 (a flat 2^-9 |ref| is not a bound: 1 + 2^-8 - eps rounds to 1), at most u |ref| for fp32.
"""
import numpy as np
import torch

U = 2.0 ** -24
EXP_ERR = 2.0 ** -23  # expf, 1 ulp (HIP math API reference)


def bf16_round(x):
    """float array -> the nearest bf16 values (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def nearest_patch(size, p, s, n):
    """i0 of every pixel 0 .. size-1: clamp(floor_div(2Y + 1 - p + s, 2s), 0, n - 1), integers"""
    Y = np.arange(size, dtype=np.int64)
    return np.clip((2 * Y + 1 - p + s) // (2 * s), 0, n - 1)  # (numpy's // is floor division)


def coefficients(s, sigma_spatial, sigma_range):
    """(cs, cr) as the caller computes them: in double, rounded once to fp32"""
    cs = 0.0 if np.isinf(sigma_spatial) else 1.0 / (2.0 * sigma_spatial * sigma_spatial * s * s)
    cr = 0.0 if np.isinf(sigma_range) else 1.0 / (2.0 * sigma_range * sigma_range)
    return np.float32(cs), np.float32(cr)


def guide_lowres_ref(G, p, s):
    """G [B, Cg, H, W] float32 -> g_lr [B, Cg, gh, gw] float32: the fp32 sum in ascending (ky, kx), one division"""
    G = np.asarray(G, dtype=np.float32)
    H, W = G.shape[2:]
    gh, gw = (H - p) // s + 1, (W - p) // s + 1
    acc = np.zeros(G.shape[:2] + (gh, gw), dtype=np.float32)
    for ky in range(p):
        for kx in range(p):
            acc = acc + G[:, :, ky:ky + (gh - 1) * s + 1:s, kx:kx + (gw - 1) * s + 1:s]
    return acc / np.float32(p * p)


def upsample_ref(F, G, p, s, r, cs, cr, conf=None, box=None, out_bf16=False, drop_lo=False, want_scale=False):
    """F [B, gh, gw, C] (bf16-representable values), G [B, Cg, H, W] float32 (the guide's values), cs / cr float32.
    Returns (out float32 [B, hb, wb, C], info): info["Z"] float64 [B, hb, wb], info["acc"] the numerators, info["exact"]
    the float64 result before any rounding, info["tmax"], info["scale"] = S (want_scale).
    drop_lo: the sum with w_hi alone (what a kernel without the lo operand would compute)."""
    F = np.asarray(F, dtype=np.float64)
    G = np.asarray(G, dtype=np.float32)
    B, gh, gw, C = F.shape
    Cg, H, W = G.shape[1:]
    assert H == p + (gh - 1) * s and W == p + (gw - 1) * s
    y0, x0, y1, x1 = box if box is not None else (0, 0, H, W)
    glr = guide_lowres_ref(G, p, s)
    cs, cr = np.float32(cs), np.float32(cr)
    Y = np.arange(y0, y1, dtype=np.int64)[:, None]
    X = np.arange(x0, x1, dtype=np.int64)[None, :]
    i0 = nearest_patch(H, p, s, gh)[y0:y1][:, None]
    j0 = nearest_patch(W, p, s, gw)[x0:x1][None, :]
    hb, wb = y1 - y0, x1 - x0
    out = np.zeros((B, hb, wb, C), dtype=np.float32)
    Zs = np.zeros((B, hb, wb))
    accs = np.zeros((B, hb, wb, C))
    exact = np.zeros((B, hb, wb, C))
    scale = np.zeros((B, hb, wb, C)) if want_scale else None
    tmax = 0.0
    half = np.float32(0.5)
    for b in range(B):
        acc = np.zeros((hb, wb, C))
        sab = np.zeros((hb, wb, C)) if want_scale else None
        Z = np.zeros((hb, wb))
        for a in range(-r, r + 1):
            for bb in range(-r, r + 1):
                i, j = i0 + a, j0 + bb
                inside = (i >= 0) & (i < gh) & (j >= 0) & (j < gw) & np.ones((hb, wb), dtype=bool)
                ic, jc = np.clip(i, 0, gh - 1) + 0 * j, np.clip(j, 0, gw - 1) + 0 * i
                dy = (2 * Y + 1 - p - 2 * s * i).astype(np.float32) * half + np.float32(0) * X.astype(np.float32)
                dx = (2 * X + 1 - p - 2 * s * j).astype(np.float32) * half + np.float32(0) * Y.astype(np.float32)
                ts = -((dy * dy + dx * dx) * cs)
                dist2 = np.zeros((hb, wb), dtype=np.float32)
                for g in range(Cg):
                    d = G[b, g, y0:y1, x0:x1] - glr[b, g][ic, jc]
                    dist2 = dist2 + d * d
                tr = -(dist2 * cr)
                t = ts + tr
                assert t.dtype == np.float32
                live = inside & ~(t < np.float32(-64.0))
                if live.any():
                    tmax = max(tmax, float(np.abs(t[live]).max()))
                w = np.where(live, np.exp(np.where(live, t, 0).astype(np.float64)), 0.0)
                if conf is not None:
                    w = w * np.where(inside, np.asarray(conf, dtype=np.float64)[b][ic, jc], 0.0)
                w32 = w.astype(np.float32)
                hi = bf16_round(w32)
                lo = bf16_round(w32 - hi)
                ws = hi.astype(np.float64) if drop_lo else hi.astype(np.float64) + lo.astype(np.float64)
                Fq = F[b][ic, jc]  # [hb, wb, C]
                acc += ws[:, :, None] * Fq
                if want_scale:
                    sab += w[:, :, None] * np.abs(Fq)
                Z += w
        zero = Z == 0
        Zd = np.where(zero, 1.0, Z)
        res = np.where(zero[:, :, None], F[b][i0 + 0 * j0, j0 + 0 * i0], acc / Zd[:, :, None])
        out[b] = res.astype(np.float32)
        exact[b] = res
        Zs[b] = Z
        accs[b] = acc
        if want_scale:
            scale[b] = np.where(zero[:, :, None], 0.0, sab / Zd[:, :, None])
    if out_bf16:
        out = bf16_round(out)
    return out, {"Z": Zs, "acc": accs, "exact": exact, "tmax": tmax, "scale": scale}


def half_ulp(x, bits):
    """half an ulp of a format with `bits` significant bits in the binade of each |x| (0 for x == 0)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)  # x = m 2^e, 0.5 <= m < 1: the binade is [2^(e-1), 2^e), its ulp 2^(e - bits)
    return np.where(x > 0, np.ldexp(0.5, e - bits), 0.0)


def bound(exact, scale, r, tmax, out_bf16, conf=True):
    """entry-wise bound of |kernel - exact| (module docstring); exact = info["exact"], scale = info["scale"]"""
    nwin = (2 * r + 1) ** 2
    K = 2 * 16 * ((nwin + 15) // 16)
    e_w = 3 * U * tmax + EXP_ERR + (U if conf else 0.0)
    rel = 2 * e_w + 2.0 ** -16 + K * U + nwin * U + U
    return scale * rel + half_ulp(exact, 8 if out_bf16 else 24)


def all_ones_ref(F, p, s, r, H, W, box=None):
    """the all-weights-one case by avg_pool2d and a gather: F [B, gh, gw, C] -> float32 [B, hb, wb, C]"""
    Ft = torch.from_numpy(np.asarray(F, dtype=np.float64)).permute(0, 3, 1, 2)
    m = torch.nn.functional.avg_pool2d(Ft, 2 * r + 1, stride=1, padding=r, count_include_pad=False).permute(0, 2, 3, 1)
    gh, gw = F.shape[1:3]
    y0, x0, y1, x1 = box if box is not None else (0, 0, H, W)
    i0 = torch.from_numpy(nearest_patch(H, p, s, gh)[y0:y1])
    j0 = torch.from_numpy(nearest_patch(W, p, s, gw)[x0:x1])
    return m[:, i0][:, :, j0].float().numpy()
