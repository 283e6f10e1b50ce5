"""Float64 restatement of vdr_op_window_vote's definition (include/vdr.h), the entry-wise bound between it and any fp32
evaluation of that definition, and a dense restatement of DINO's label propagation step (TEST HELPER), for
tests/test_window_vote_cpu.py, tests/test_window_vote_gpu.py and tests/test_propagate_volume_gpu.py.

Definition, for cost [P, S, t, W * W] fp32 and src [P, S, t, C] fp32 (finite, non-negative) on a gh x gw grid:
    candidates of query i   the (s, w) whose slot lies inside the grid (local_corr_ref.window), value cost[p, s, i, w],
                            patch j = (qy + dy) * gw + (qx + dx)
    order                   greater value, then lower s, then lower w; the neighbours m = 0 .. k-1 are the first k
    e_m                     exp((v_m - v_0) / T) (softmax) or 1 (uniform), T the fp32 value of the temperature
    scores[p, i, c]         sum_m e_m src[p, s_m, j_m, c] / sum_m e_m;   idx = s_m * t + j_m, val = v_m
The SELECTION is taken from exact comparisons of the fp32 values (float64 holds every fp32 value, and a stable sort of the
[S * W * W] row, sources concatenated in order, breaks ties by s then w): it has no error, so idx and val are compared
exactly.  `vote` evaluates the scores in float64.

The bound (`bound`) between the float64 scores and an fp32 evaluation as the header states it, u = 2^-24, term by term:
  * the exponent a_m = (v_m - v_0) * (1 / T): 1 / T rounded once (u), the subtraction once (u), the product once (u):
    a relative error of the argument of 3 u (1.01 covers the second-order terms), |da_m| <= 3.03 u |v_m - v_0| / T.  An absolute
    error da in the argument is the relative error expm1(|da|) of the exponential;
  * the exponential itself: at most 1 ulp by the header, which is at most 2^-23 relative;  together
    d_m = expm1(3.03 u |a_m|) + 2^-23 * 1.01, and d_0 = 0: e_0 is exactly 1.  D = max_m d_m;
  * a weighted mean of NON-NEGATIVE terms whose weights each move by a relative (1 + d), |d| <= D, stays inside
    [(1 - D) / (1 + D), (1 + D) / (1 - D)] times itself: |ds| <= s * 2 D / (1 - D);
  * the fp32 sums: k products (u each), k - 1 additions in each sum and one division -- 2 k roundings on sums without
    cancellation: |ds| <= s * 2 k u * 1.01;
  * underflow: an e_m below 2^-126 may be flushed or lose bits, a product likewise: absolute terms far below 2^-120 each,
    granted as k * 2^-120 * (1 + max_m src).
  bound = s * (2 D / (1 - D) + 2.02 k u) + k * 2^-120 * (1 + max_m src[.., c]).   Uniform weights: D = 0.

DINO's form (`dino_dense`, float64), as eval_video_segmentation's label_propagation states it: aff = exp(cost / T) on the
window (0 outside the grid), per query everything below its k-th largest value set to 0 -- so everything TIED with the k-th
stays, which is where the op's "exactly k" departs --, the column normalised to sum 1, scores = src^T @ aff as a dense
[S * t] product.  exp(v / T) / sum exp(v / T) is exp((v - v_0) / T) / sum exp((v - v_0) / T): on a row without a tie at the k-th
value the two forms are the same number, and differ in float64 by a few 1e-16."""
import numpy as np

import local_corr_ref as lref

U = 2.0 ** -24
EXP_REL = 2.0 ** -23  # 1 ulp, the error include/vdr.h states for the exponential


def _f64(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a).astype(np.float64)


def radius_of(cost) -> int:
    return {(2 * r + 1) ** 2: r for r in range(1, 9)}[int(cost.shape[-1])]


def rows(cost, grid):
    """cost [P, S, t, WW] -> ([P, t, S * WW] float64 with -inf at the slots outside the grid, j [t, WW])"""
    c = _f64(cost)
    P, S, t, WW = c.shape
    j, ok = lref.window(grid[0], grid[1], radius_of(c))
    return np.where(ok[None, None], c, -np.inf).transpose(0, 2, 1, 3).reshape(P, t, S * WW), j


def select(cost, grid, k: int):
    """(e [P, t, k] int64: the neighbours as row elements s * WW + w, best first; idx [P, t, k] int32 = s * t + j; val [P, t, k]
    float64, exactly the fp32 values)"""
    r, j = rows(cost, grid)
    t, WW = j.shape
    e = np.argsort(-r, axis=-1, kind="stable")[..., :k]
    val = np.take_along_axis(r, e, -1)
    assert np.isfinite(val).all(), "a slot outside the grid was selected: k exceeds a patch's candidates"
    idx = (e // WW) * t + j[np.arange(t)[None, :, None], e % WW]
    return e, idx.astype(np.int32), val


def _weights(val: np.ndarray, weights: str, temperature: float) -> np.ndarray:
    if weights == "uniform":
        return np.ones_like(val)
    return np.exp((val - val[..., :1]) / float(np.float32(temperature)))


def vote(cost, src, grid, k: int, weights: str = "softmax", temperature: float = 0.1):
    """float64 (scores [P, t, C], labels [P, t] int32: the lowest class of the largest score, idx, val)"""
    s = _f64(src)
    P, S, t, C = s.shape
    _, idx, val = select(cost, grid, k)
    near = s.reshape(P, S * t, C)[np.arange(P)[:, None, None], idx]  # [P, t, k, C]
    e = _weights(val, weights, temperature)
    scores = (e[..., None] * near).sum(-2) / e.sum(-1)[..., None]
    return scores, scores.argmax(-1).astype(np.int32), idx, val  # (numpy's argmax is the FIRST maximum)


def bound(cost, src, grid, k: int, weights: str = "softmax", temperature: float = 0.1) -> np.ndarray:
    """[P, t, C]: the bound of the module docstring"""
    s = _f64(src)
    P, S, t, C = s.shape
    _, idx, val = select(cost, grid, k)
    near = s.reshape(P, S * t, C)[np.arange(P)[:, None, None], idx]
    e = _weights(val, weights, temperature)
    scores = (e[..., None] * near).sum(-2) / e.sum(-1)[..., None]
    if weights == "uniform":
        D = np.zeros(val.shape[:-1])
    else:
        a = np.abs(val - val[..., :1]) / float(np.float32(temperature))
        d = np.where(a > 0, np.expm1(3.03 * U * a) + 1.01 * EXP_REL, 0.0)
        D = np.minimum(d.max(-1), 0.5)
    return scores * (2.0 * D / (1.0 - D) + 2.02 * k * U)[..., None] + k * 2.0 ** -120 * (1.0 + near.max(-2))


def knn_vote_bound(val, scores: np.ndarray, weights: str, temperature: float) -> np.ndarray:
    """The bound granted to vdr.knn.vote against the float64 scores [.., C] of the same neighbours, val [.., k]: its weights
    are torch's softmax of val / T -- local_corr_ref's weight error eps_w = u (4 Z + 2 A + 16 + k) for the same construction,
    Z = max |val / T|, A = max - min of val / T --, then k products and k - 1 additions: (eps_w + k u), doubled as there.
    Uniform weights are exact counts and one division: eps_w = 0."""
    z = _f64(val) / float(temperature)
    k = z.shape[-1]
    eps = U * (4.0 * np.abs(z).max(-1) + 2.0 * (z.max(-1) - z.min(-1)) + 16.0 + k) if weights == "softmax" else np.zeros(z.shape[:-1])
    return 2.0 * scores * (eps + k * U)[..., None]


def margin_clear(scores: np.ndarray, bnd: np.ndarray) -> np.ndarray:
    """[P, t] bool: the two largest scores differ by more than twice the (largest) bound, so every evaluation inside the
    bound has the same arg-max; rows of one class are clear"""
    if scores.shape[-1] == 1:
        return np.ones(scores.shape[:-1], bool)
    top = np.sort(scores, -1)
    return top[..., -1] - top[..., -2] > 2.0 * bnd.max(-1)


def dino_dense(cost, src, grid, k: int, temperature: float = 0.1):
    """DINO's label propagation step as dense algebra -> (scores [P, t, C] float64, no_tie [P, t] bool: the k-th largest
    affinity of the row is strictly greater than the next one, so "at least the k-th" keeps exactly k)"""
    s = _f64(src)
    P, S, t, C = s.shape
    r, j = rows(cost, grid)
    WW = j.shape[1]
    aff = np.exp(r / float(np.float32(temperature)))  # exp(-inf) = 0: the window mask
    ranked = -np.sort(-aff, axis=-1)
    kth = ranked[..., k - 1:k]
    no_tie = ranked[..., k - 1] > ranked[..., k] if ranked.shape[-1] > k else np.ones(ranked.shape[:-1], bool)
    aff = np.where(aff >= kth, aff, 0.0)
    aff = aff / aff.sum(-1, keepdims=True)
    # scatter the [S * WW] row to the dense [S * t] column of the affinity matrix (out-of-grid slots carry 0 to patch 0)
    e = np.arange(S * WW)
    col = (e // WW)[None, :] * t + j[:, e % WW]  # [t, S * WW]
    dense = np.zeros((P, t, S * t))
    for p in range(P):
        np.add.at(dense[p], (np.arange(t)[:, None], col), aff[p])
    return dense @ s.reshape(P, S * t, C), no_tie


def designed(P: int, S: int, grid, r: int, C: int, seed: int, values=(0.0, 2.0, 4.0), dyadic: bool = True):
    """Seeded inputs on which an fp32 evaluation is exact: cost drawn from `values` (with T = 0.01 a gap of 2 is a factor
    exp(-200) < 2^-126... the weight of everything below the row's best value is far below half an ulp of any sum, and the
    best values weigh exactly 1), -inf outside the grid as local_correlation writes it; src one-hot (dyadic=False) or
    multiples of 1/8 in [0, 1] (dyadic=True).  Returns torch (cost [P, S, t, WW] fp32, src [P, S, t, C] fp32)."""
    import torch
    gh, gw = grid
    t, WW = gh * gw, (2 * r + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(values, dtype=torch.float32)
    cost = vals[torch.randint(0, len(values), (P, S, t, WW), generator=g)]
    _, ok = lref.window(gh, gw, r)
    cost = torch.where(torch.from_numpy(ok)[None, None], cost, torch.tensor(float("-inf")))
    if dyadic:
        src = torch.randint(0, 9, (P, S, t, C), generator=g).float() / 8.0
    else:
        src = torch.nn.functional.one_hot(torch.randint(0, C, (P, S, t), generator=g), C).float()
    return cost.contiguous(), src.contiguous()


def random_inputs(P: int, S: int, grid, r: int, C: int, seed: int):
    """Seeded inputs like the real ones: cosines in [-1, 1] rounded to fp32 (continuous, so ties have probability ~0), -inf
    outside the grid; src rows non-negative, summing to 1"""
    import torch
    gh, gw = grid
    t, WW = gh * gw, (2 * r + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    cost = torch.rand((P, S, t, WW), generator=g) * 2.0 - 1.0
    _, ok = lref.window(gh, gw, r)
    cost = torch.where(torch.from_numpy(ok)[None, None], cost, torch.tensor(float("-inf")))
    src = torch.rand((P, S, t, C), generator=g)
    return cost.contiguous(), (src / src.sum(-1, keepdim=True)).contiguous()
