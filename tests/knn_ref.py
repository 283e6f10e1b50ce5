"""Float64 statement of exact k nearest neighbours between two descriptor maps -- the scores a fused top-k kernel beside
vdr_op_nn_cosine has to return --, the entry-wise bounds between it and any fp32 evaluation, and the acceptance rule for random
inputs; for tests/test_knn_cpu.py and tests/golden/make_golden_knn.py.  The library has no such kernel yet (vdr.knn holds the
vote that consumes its output); the bounds and the rule are here so that the kernel's tests need not invent them.

Definition, for queries Q [tq, d] and candidates C [tc, d] (values exactly representable in bf16), ss(v) = sum_c v_c^2:
    cosine  s(i, j) = (dot(q_i, c_j) * rn(q_i)) * rn(c_j), rn(v) = 1 / max(sqrt(ss(v)), 1e-8)   better: greater, then lower j
    l2      s(i, j) = max(ss(q_i) + ss(c_j) - 2 dot(q_i, c_j), 0)                              better: smaller, then lower j
    exclude_self: candidate j == i is not eligible.  Output: the k best eligible candidates of every query, best first.
Here every step is float64 (`scores`), and the order is a STABLE sort of the cost (-s for cosine, s for l2) along j
(`topk`): equal costs stay in index order.

Bounds, u = 2^-24 (fp32 unit roundoff).  Cosine: nn_cosine_ref.bound (the same arithmetic).  l2 (`bound`), with
A_ij = sum_c |q_ic c_jc|:
  * ss(q), ss(c): fp32 sums of d exact non-negative terms in any order: <= d u ss each.
  * their sum: one rounding, u (ss_q + ss_c).
  * dot: d exact products summed in fp32 in any order: <= d u A.  It enters with the factor 2 (exact).
  * the fused multiply-add rounds once: u |ss_q + ss_c - 2 dot| <= u (ss_q + ss_c + 2 |dot|).
  * the clamp at 0 moves the value towards the true one (which is >= 0): no error.
  Sum: d u (ss_q + ss_c + 2 A) + u (2 (ss_q + ss_c) + 2 |dot|) <= d u (ss_q + ss_c + 2 A) + 4 u (ss_q + ss_c + 2 |dot|) (second-
  order terms).  bound = 2 * that, doubled for margin.
Checked on the CPU (tests/test_knn_cpu.py prints the ratios): an fp32 emulation with another summation order stays far
below both.

Designed inputs: nn_cosine_ref.designed (16 entries of +-1 per row): every cosine is a multiple of 1/16 and every squared
distance the integer 32 - 2 dot, so any fp32 evaluation equals the float64 one bit for bit, ties included.

Planted clusters (`planted`): 7 centres ~ N(0, 1)^d, points = centre + 0.5 N(0, 1)^d, every value rounded to bf16."""
import numpy as np
import torch

import nn_cosine_ref as nref

U = nref.U
METRICS = ("cosine", "l2")


def scores(q, c, metric: str) -> np.ndarray:
    """q [P, tq, d], c [P, tc, d] -> float64 s [P, tq, tc] in the definition's association"""
    if metric == "cosine":
        return nref.similarity(q, c)
    q, c = nref._f64(q), nref._f64(c)
    ssq, ssc = (q * q).sum(-1), (c * c).sum(-1)
    return np.maximum(ssq[:, :, None] + ssc[:, None, :] - 2.0 * np.einsum("pic,pjc->pij", q, c), 0.0)


def bound(q, c, s: np.ndarray, metric: str) -> np.ndarray:
    """entry-wise bound [P, tq, tc] between the float64 score s and an fp32 evaluation of the definition"""
    if metric == "cosine":
        return nref.bound(q, c, s)
    q, c = nref._f64(q), nref._f64(c)
    d = q.shape[-1]
    ss = (q * q).sum(-1)[:, :, None] + (c * c).sum(-1)[:, None, :]
    A = np.einsum("pic,pjc->pij", np.abs(q), np.abs(c))
    dot = np.einsum("pic,pjc->pij", q, c)
    return 2.0 * (d * U * (ss + 2.0 * A) + 4.0 * U * (ss + 2.0 * np.abs(dot)))


def cost(s: np.ndarray, metric: str, exclude_self: bool = False) -> np.ndarray:
    """lower is better: -s (cosine) or s (l2); the excluded diagonal at +inf"""
    c = -s if metric == "cosine" else s.copy()
    if exclude_self:
        i = np.arange(min(c.shape[-2], c.shape[-1]))
        c[..., i, i] = np.inf
    return c


def topk(s: np.ndarray, k: int, metric: str, exclude_self: bool = False):
    """s [..., tq, tc] -> (val [..., tq, k] float64, idx [..., tq, k] int32): a stable sort of (cost, index)"""
    order = np.argsort(cost(s, metric, exclude_self), axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(s, order, -1), order.astype(np.int32)


def clear_rows(s: np.ndarray, b: np.ndarray, k: int, metric: str, exclude_self: bool = False) -> np.ndarray:
    """bool [..., tq]: rows on which no fp32 evaluation within the bounds can change the first k indices or their order --
    the first k + 1 float64 costs are pairwise separated by more than the sum of their bounds, and so is the k-th from
    every later one"""
    c = cost(s, metric, exclude_self)
    order = np.argsort(c, axis=-1, kind="stable")
    cs, bs = np.take_along_axis(c, order, -1), np.take_along_axis(b, order, -1)
    n = c.shape[-1] - int(exclude_self)  # eligible candidates
    m = min(k + 1, n)
    ok = ((cs[..., 1:m] - cs[..., :m - 1]) > (bs[..., 1:m] + bs[..., :m - 1])).all(-1)
    if n > k:
        with np.errstate(invalid="ignore"):
            ok &= ((cs[..., k:n] - bs[..., k:n]) > (cs[..., k - 1:k] + bs[..., k - 1:k])).all(-1)
    return ok


def check_near_tie_tolerant(s: np.ndarray, b: np.ndarray, got_val: np.ndarray, got_idx: np.ndarray, metric: str,
                            exclude_self: bool = False, what="") -> float:
    """The rule for random inputs, along the last axis of s [..., tq, tc] with got_val / got_idx [..., tq, k]:
      * the returned indices are distinct, in range and eligible;
      * every value is within the bound of the float64 score at its index;
      * the returned worst is no worse than the float64 k-th best by more than the two bounds;
      * on clear rows (clear_rows) the indices equal the float64 ones, in order.
    Returns the share of clear rows."""
    tq, tc = s.shape[-2:]
    k = got_idx.shape[-1]
    assert got_idx.dtype == np.int32 and got_val.dtype == np.float32, what
    assert got_idx.min() >= 0 and got_idx.max() < tc, what
    srt = np.sort(got_idx, -1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), (what, "repeated index")
    if exclude_self:
        assert (got_idx != np.arange(tq).reshape((1,) * (got_idx.ndim - 2) + (tq, 1))).all(), (what, "own index returned")
    gi = got_idx.astype(np.int64)
    s_got, b_got = np.take_along_axis(s, gi, -1), np.take_along_axis(b, gi, -1)
    err = np.abs(got_val.astype(np.float64) - s_got)
    print(f"{what}: max |val - s| {err.max():.3e}, max err / bound {(err / b_got).max():.3e}")
    assert (err <= b_got).all(), (what, float((err / b_got).max()))
    c = cost(s, metric, exclude_self)
    order = np.argsort(c, axis=-1, kind="stable")
    kth = order[..., k - 1:k]
    c_kth, b_kth = np.take_along_axis(c, kth, -1)[..., 0], np.take_along_axis(b, kth, -1)[..., 0]
    c_got = np.take_along_axis(c, gi, -1)
    worst = c_got.argmax(-1)[..., None]
    c_worst, b_worst = np.take_along_axis(c_got, worst, -1)[..., 0], np.take_along_axis(b_got, worst, -1)[..., 0]
    assert (c_worst <= c_kth + b_kth + b_worst).all(), (what, float((c_worst - c_kth).max()))
    clear = clear_rows(s, b, k, metric, exclude_self)
    assert (got_idx[clear] == order[..., :k][clear]).all(), (what, "order on clear rows")
    return float(clear.mean())


def planted(n: int, d: int, seed: int, centres_seed: int = 0, n_centres: int = 7, noise: float = 0.5):
    """(points [n, d] fp32 holding bf16 values, labels [n] int64): planted clusters.  The centres depend on centres_seed and
    d only, so queries and candidates drawn with different seeds share them."""
    centres = np.random.default_rng(1000003 * centres_seed + d).standard_normal((n_centres, d))
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_centres, n)
    x = centres[labels] + noise * rng.standard_normal((n, d))
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float(), torch.from_numpy(labels.astype(np.int64))


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    """bf16-exact fp32 tensor -> its bf16 bit patterns as uint16 (how the golden files store descriptors)"""
    assert torch.equal(x.to(torch.bfloat16).float(), x.float())
    return (x.float().contiguous().view(torch.int32).numpy() >> 16).astype(np.uint16)


def from_bf16_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy((a.astype(np.int32) << 16)).view(torch.float32)


def fp32_other_order(q, c, metric: str) -> np.ndarray:
    """an fp32 evaluation of the definition with ANOTHER summation order than the kernel's (numpy's pairwise / BLAS sums):
    what the bounds must cover"""
    q, c = np.asarray(nref._f64(q), np.float32), np.asarray(nref._f64(c), np.float32)
    dot = np.einsum("pic,pjc->pij", q[..., ::-1], c[..., ::-1]).astype(np.float32)
    ssq, ssc = (q * q).sum(-1, dtype=np.float32), (c * c).sum(-1, dtype=np.float32)
    if metric == "cosine":
        rq = np.float32(1) / np.maximum(np.sqrt(ssq), np.float32(1e-8))
        rc = np.float32(1) / np.maximum(np.sqrt(ssc), np.float32(1e-8))
        return (dot * rq[:, :, None]) * rc[:, None, :]
    return np.maximum((ssq[:, :, None] + ssc[:, None, :]) - np.float32(2) * dot, np.float32(0))
