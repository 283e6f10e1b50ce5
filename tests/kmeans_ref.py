"""Float64 restatement of vdr_op_kmeans_assign's and vdr_op_kmeans_update's definitions (include/vdr.h), of the Lloyd loop,
the maximin initialisation and the saliency vote of vdr/kmeans.py, and the entry-wise bounds between the restatement and
any fp32 evaluation.  For tests/test_kmeans_cpu.py, tests/test_kmeans_gpu.py, tests/test_kmeans_model_gpu.py and
tests/golden/make_golden_kmeans.py.

Definition, for X [R, d] (values exactly representable in bf16) and fp32 centroids C [k, d]:
    c_hi = bf16_rn(c), c_lo = bf16_rn(c - c_hi);  s(i, j) = dot(x_i, c_hi_j) + dot(x_i, c_lo_j);  cc_j = sum c_j^2 (of the fp32
    centroid), xx_i = sum x_i^2;  h(i, j) = cc_j - 2 s(i, j);  label_i = argmin_j h, the lowest j on a tie;
    min_dist_i = max(xx_i + h(i, label_i), 0);  inertia = sum_i min_dist_i.
    update: centroid_j = (sum of the rows labelled j) / count_j, rounded to fp32; an empty cluster keeps its centroid.
Here every step is float64 (`scores`, `assign`, `update`, `lloyd`); argmin is numpy's: the FIRST index of the minimum.

The bounds, with u = 2^-24 and g(n) = n u / (1 - n u) (the rigorous constant of an fp32 sum of n terms in ANY order):
  * s: the products of two bf16 values are exact in fp32.  The header states the order: one accumulator, 16 channels per MFMA,
    channels ascending, per 16 channels the block of c_hi products and then the block of c_lo products.  One MFMA adds 16 exact
    products to the accumulator; whatever its internal order, 17 values summed by operations no worse than correctly rounded
    fp32 additions err by at most g(17) (|S_before| + sum |t| of the block) (assumed of the hardware, and doubled here for an
    adder that truncates instead of rounding).  Summed over the 2 d / 16 blocks, with the partial sums S_before taken from the
    float64 evaluation in that order:  |ds| <= 2 g(17) (A_ij + sum_blocks |S_before|),  A_ij = sum_c |x_ic| (|c_hi_jc| + |c_lo_jc|).
    For zero-mean data the partial sums grow like a random walk, which is what makes this bound some 20 times tighter than
    the order-free g(2 d) A_ij at d = 416 -- and the golden maps' margin condition attainable there (README_kmeans.md).
  * cc: d squares, each rounded (u), then summed: |dcc| <= g(d + 1) cc_j.  xx: exact squares: |dxx| <= g(d) xx_i.
  * h = cc - 2 s, one rounding: |dh| <= 2 |ds| + g(d + 1) cc_j + u (|h| + that)                 (`s_bound`, `h_bound`)
  * min_dist = max(xx + h, 0), one rounding (max is 1-Lipschitz): |dmd| <= dh + g(d) xx_i + u (|xx + h| + those)
  * inertia, R terms: |dI| <= sum_i dmd_i + g(R) sum_i (md_i + dmd_i)
  * centroid: a sum of n_j exact fp32 values, then one division: |dc| <= g(n_j) sum_i |x_ic| / n_j + u |c| (first order in
    the second term; the bound adds u times the first term)
  What hi + lo leaves of the fp32 centroid, |c - c_hi - c_lo| <= 2^-17 |c| (two roundings to 8 bits: 2^-9 * 2^-9 = 2^-18, half
  an ulp of the second), is part of the DEFINITION: it separates s from the dot product with the fp32 centroid (sklearn's),
  `split_residual_bound` = 2^-17 sum_c |x_ic c_jc| on s, not the restatement from the kernel.

fp32 emulation (`assign_fp32`, `update_fp32`, `lloyd_fp32`): the same steps with every stated rounding carried out in
numpy float32 and the stated orders of cc / xx (`sumsq_lanes`) and of the inertia (`sum_colmean_order`); s and the cluster
sums are formed in float64 and rounded once.  On designed inputs (`designed`: x integer in [-4, 4], centroids multiples of
2^-8 below 8 in magnitude, so hi + lo is exact and every partial sum of s and of the cluster sums is exact in fp32) that is
the kernels' result bit for bit."""
import numpy as np
import torch

U = 2.0 ** -24
COV_CHUNK = 1024   # VDR_COV_CHUNK: the inertia's chunk
KMEANS_CHUNK = 256  # VDR_KMEANS_CHUNK


def g(n):
    return n * U / (1.0 - n * U)


def _f64(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().to(torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def bf16_rn(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even to bf16 of an array of fp32-representable values, returned as float64"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float64).numpy()


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """values exactly representable in bf16 -> their uint16 bit patterns"""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    bits = (a32.view(np.uint32) >> 16).astype(np.uint16)
    assert (from_bf16_bits(bits) == a32).all()
    return bits


def from_bf16_bits(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split(c) -> tuple:
    """fp32 centroids -> (c_hi, c_lo) as float64"""
    c = _f64(c)
    hi = bf16_rn(c)
    return hi, bf16_rn(c - hi)


def scores(x, c):
    """x [R, d], c [k, d] -> (h [R, k], xx [R], cc [k], s [R, k]) in float64"""
    x, c = _f64(x), _f64(c)
    hi, lo = split(c)
    s = x @ hi.T + x @ lo.T
    cc = (c * c).sum(-1)
    return cc[None, :] - 2.0 * s, (x * x).sum(-1), cc, s


def s_bound(x, c) -> np.ndarray:
    """|ds| [R, k]: the blocks of 16 channels in the kernel's order (hi block, lo block, channels ascending)"""
    x = _f64(x)
    hi, lo = split(c)
    R, d = x.shape
    k = hi.shape[0]
    xb = x.reshape(R, d // 16, 16)
    S = np.zeros((R, k))
    walk = np.zeros((R, k))  # sum over the blocks of |S_before|
    A = np.zeros((R, k))
    for b in range(d // 16):
        for op in (hi, lo):
            ob = op.reshape(k, d // 16, 16)[:, b]
            walk += np.abs(S)
            S += xb[:, b] @ ob.T
            A += np.abs(xb[:, b]) @ np.abs(ob).T
    return 2.0 * g(17) * (A + walk) * 1.001  # (1.001: S_before is the float64 value, not the kernel's -- a second-order term)


def h_bound(x, c, h=None) -> np.ndarray:
    x, c = _f64(x), _f64(c)
    if h is None:
        h = scores(x, c)[0]
    b = 2.0 * s_bound(x, c) + g(x.shape[-1] + 1) * (c * c).sum(-1)[None, :]
    return b + U * (np.abs(h) + b)


def split_residual_bound(x, c) -> np.ndarray:
    return 2.0 ** -17 * (np.abs(_f64(x)) @ np.abs(_f64(c)).T)


def assign(x, c, prev=None):
    """-> dict(labels int32 [R], min_dist [R], inertia, changed, margin [R] (second-best h minus best; inf when k == 1), h)"""
    h, xx, _, _ = scores(x, c)
    lab = h.argmin(-1)
    best = np.take_along_axis(h, lab[:, None], 1)[:, 0]
    md = np.maximum(xx + best, 0.0)
    if h.shape[1] > 1:
        margin = np.partition(h, 1, axis=-1)[:, 1] - best
    else:
        margin = np.full(h.shape[0], np.inf)
    prev = np.full(h.shape[0], -1) if prev is None else np.asarray(prev)
    return dict(labels=lab.astype(np.int32), min_dist=md, inertia=md.sum(), changed=int((prev != lab).sum()), margin=margin, h=h)


def assign_bounds(x, c, a: dict):
    """-> (label_bound [R]: a row whose margin exceeds it has its float64 label in any fp32 evaluation; min_dist bound [R];
    inertia bound)"""
    x = _f64(x)
    hb = h_bound(x, c, a["h"])
    lab = a["labels"].astype(np.int64)
    hb_best = np.take_along_axis(hb, lab[:, None], 1)[:, 0]
    xx = (x * x).sum(-1)
    d = x.shape[-1]
    b = hb_best + g(d) * xx
    mdb = b + U * (np.abs(a["min_dist"]) + b)
    ib = mdb.sum() + g(x.shape[0]) * (a["min_dist"] + mdb).sum()
    return hb_best + hb.max(-1), mdb, ib


def update(x, labels, c_prev):
    """-> (centroids [k, d] float64: the mean rounded to fp32, an empty cluster keeps c_prev; counts int32 [k])"""
    x, c_prev = _f64(x), _f64(c_prev)
    k = c_prev.shape[0]
    out = c_prev.copy()
    counts = np.zeros(k, np.int32)
    for j in range(k):
        m = np.asarray(labels) == j
        counts[j] = m.sum()
        if counts[j]:
            out[j] = (x[m].sum(0) / counts[j]).astype(np.float32)
    return out, counts


def centroid_bound(x, labels, cent) -> np.ndarray:
    x, cent = _f64(x), _f64(cent)
    b = np.zeros_like(cent)
    for j in range(cent.shape[0]):
        m = np.asarray(labels) == j
        n = int(m.sum())
        if n:
            first = g(n) * np.abs(x[m]).sum(0) / n
            b[j] = first + U * (np.abs(cent[j]) + first)
    return b


def lloyd(x, init, max_iter=300, step=None):
    """The loop of vdr.kmeans.fit in float64: assign + update until an assign changes no label.  step(it, a): called with
    every assignment (the golden generator's margin check).  -> dict(labels, centroids, inertia, counts, iters, converged)"""
    c = _f64(np.asarray(_f64(init), dtype=np.float32))
    prev, counts, a, it = None, None, None, 0
    converged = False
    for it in range(1, max_iter + 1):
        a = assign(x, c, prev)
        if step is not None:
            step(it, a, c)
        if a["changed"] == 0:
            converged = True
            break
        prev = a["labels"]
        c, counts = update(x, prev, c)
    return dict(labels=a["labels"], centroids=c, inertia=a["inertia"], counts=counts, iters=it, converged=converged)


# ---- fp32 emulation ---------------------------------------------------------------------------------
def sumsq_lanes(v: np.ndarray) -> np.ndarray:
    """cc / xx in the stated order, in float32: v [n, d] float32 -> [n]; lane l of 64 sums the channels 8l .. 8l+7, 512 + 8l ..
    ascending (each square rounded), then the xor butterfly 32, 16, ... 1"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    n, d = v.shape
    M = (d + 511) // 512
    p = np.zeros((n, M * 512), np.float32)
    p[:, :d] = v
    p = p.reshape(n, M, 64, 8)
    ss = np.zeros((n, 64), np.float32)
    for m in range(M):
        for e in range(8):
            ss = (ss + p[:, m, :, e] * p[:, m, :, e]).astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = (ss + ss[:, lanes ^ o]).astype(np.float32)
    return ss[:, 0]


def sum_colmean_order(v: np.ndarray) -> np.float32:
    """col_mean's order in float32: chunks of 1024, sixteen interleaved sums folded ascending, chunk sums ascending"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    total = None
    for r0 in range(0, len(v), COV_CHUNK):
        c = np.zeros(COV_CHUNK, np.float32)
        c[:len(v[r0:r0 + COV_CHUNK])] = v[r0:r0 + COV_CHUNK]
        c = c.reshape(COV_CHUNK // 16, 16)
        lanes = np.zeros(16, np.float32)
        for i in range(c.shape[0]):
            lanes = (lanes + c[i]).astype(np.float32)
        f = lanes[0]
        for j in range(1, 16):
            f = np.float32(f + lanes[j])
        total = f if total is None else np.float32(total + f)
    return total


def assign_fp32(x, c, prev=None):
    """the assignment with every stated rounding in float32 (s formed in float64 and rounded once)"""
    x32 = np.asarray(_f64(x), np.float32)
    c32 = np.asarray(_f64(c), np.float32)
    hi, lo = split(c32)
    s = (x32.astype(np.float64) @ hi.T + x32.astype(np.float64) @ lo.T).astype(np.float32)
    cc, xx = sumsq_lanes(c32), sumsq_lanes(x32)
    h = (cc[None, :] - np.float32(2.0) * s).astype(np.float32)
    lab = h.argmin(-1)
    best = np.take_along_axis(h, lab[:, None], 1)[:, 0]
    md = np.maximum((xx + best).astype(np.float32), np.float32(0.0))
    prev = np.full(len(lab), -1) if prev is None else np.asarray(prev)
    return dict(labels=lab.astype(np.int32), min_dist=md, inertia=sum_colmean_order(md), changed=int((prev != lab).sum()))


def update_fp32(x, labels, c_prev):
    """the update with the chunk sums folded and the division in float32 (a chunk's sum formed in float64 and rounded once)"""
    x64 = _f64(x)
    out = np.asarray(_f64(c_prev), np.float32).copy()
    k = out.shape[0]
    labels = np.asarray(labels)
    counts = np.zeros(k, np.int32)
    for j in range(k):
        m = labels == j
        counts[j] = m.sum()
        if not counts[j]:
            continue
        tot = None
        for r0 in range(0, len(labels), KMEANS_CHUNK):
            part = x64[r0:r0 + KMEANS_CHUNK][m[r0:r0 + KMEANS_CHUNK]].sum(0).astype(np.float32)
            tot = part if tot is None else (tot + part).astype(np.float32)
        out[j] = (tot / np.float32(counts[j])).astype(np.float32)
    return out, counts


def lloyd_fp32(x, init, max_iter=300):
    c = np.asarray(_f64(init), np.float32)
    prev, counts, a, it, converged = None, None, None, 0, False
    for it in range(1, max_iter + 1):
        a = assign_fp32(x, c, prev)
        if a["changed"] == 0:
            converged = True
            break
        prev = a["labels"]
        c, counts = update_fp32(x, prev, c)
    return dict(labels=a["labels"], centroids=c, inertia=a["inertia"], counts=counts, iters=it, converged=converged)


# ---- inputs -----------------------------------------------------------------------------------------
def designed(R: int, k: int, d: int, seed: int):
    """(x [R, d] fp32 with integer entries in [-4, 4], centroids [k, d] fp32 multiples of 2^-8 below 8 in magnitude).  X and
    the centroids are drawn differently (a row / column swap changes the result).  Planted where the shapes have room:
    centroid 1 copied to the last centroid and, from k >= 5, to centroid 3 as well (duplicates: the lowest index wins) and
    one centroid far from every row (all entries 7.5: no row chooses it)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(R, d)).astype(np.float32)
    c = (rng.integers(-3 * 256, 3 * 256 + 1, size=(k, d)) / 256.0).astype(np.float32)
    if k >= 3:
        c[k - 1] = c[1]
    if k >= 5:
        c[3] = c[1]
        c[2] = 7.5
    return x, c


def planted(R: int, d: int, k: int, sep: float, seed: int, decay: float = 0.0):
    """a planted-cluster map: k centres drawn N(0, sep^2) per channel, rows = centre + N(0, 1), channel c scaled by
    1 / (1 + decay c) (decay > 0: a falling spectrum, as descriptors have); rounded to bf16.  -> (x [R, d] fp32 holding
    bf16 values, the planted labels)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, sep, size=(k, d))
    lab = rng.integers(0, k, size=R)
    x = (centres[lab] + rng.normal(0.0, 1.0, size=(R, d))) / (1.0 + decay * np.arange(d))[None, :]
    return bf16_rn(x).astype(np.float32), lab


def maximin(x, k: int) -> np.ndarray:
    """float64 farthest-point initialisation on one map x [R, d] -> indices [k]: the row of largest squared norm, then the row
    farthest (squared distance to the nearest chosen row) from the chosen set; ties to the lowest index"""
    x = _f64(x)
    idx = [int((x * x).sum(-1).argmax())]
    mind = np.full(x.shape[0], np.inf)
    for _ in range(1, k):
        mind = np.minimum(mind, ((x - x[idx[-1]]) ** 2).sum(-1))
        idx.append(int(mind.argmax()))
    return np.asarray(idx, np.int64)


def vote(labels, saliency, k: int, thresh: float, votes_percentage: float) -> np.ndarray:
    """labels [B, n], saliency [B, n] -> salient [k] bool: a cluster is salient when in at least votes_percentage % of the
    images the mean saliency of that image's patches in the cluster exceeds thresh (no patch: no vote)"""
    labels, sal = np.asarray(labels), _f64(saliency)
    B = labels.shape[0]
    out = np.zeros(k, bool)
    for j in range(k):
        votes = 0
        for b in range(B):
            m = labels[b] == j
            if m.any() and sal[b][m].mean() > thresh:
                votes += 1
        out[j] = votes * 100.0 >= votes_percentage * B
    return out
