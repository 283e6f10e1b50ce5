"""Float64 restatement of vdr_op_nn_cosine's definition (include/vdr.h) and the entry-wise bound between it and any fp32
evaluation, for tests/test_nn_cosine_cpu.py, tests/test_nn_cosine_gpu.py and tests/test_correspondences_gpu.py.

Definition, for X [tx, d] and Y [ty, d] (values exactly representable in bf16):
    ss(v) = sum_c v_c^2,  rn(v) = 1 / max(sqrt(ss(v)), 1e-8),  sim(i, j) = (dot(x_i, y_j) * rn(x_i)) * rn(y_j)
    row_sim[i] = max_j sim(i, j), row_idx[i] the lowest j attaining it; col_sim / col_idx the same over i.
Here every step is float64 (`similarity`), and the arg-maxima are numpy's argmax: the FIRST index of the maximum.

The bound (`bound`), with u = 2^-24 (fp32 unit roundoff), s the float64 similarity and
A_ij = sum_c |x_ic y_jc| * rn_i * rn_j:
  * dot: the products of two bf16 values are exact in fp32 (8 + 8 significand bits); an fp32 sum of d exact terms in any
    order errs by at most (d - 1) u sum|x y| to first order, <= d u sum|x y|.  Scaled by the two norms: d u A_ij.
  * rn: ss is such a sum of d non-negative terms: relative error <= d u, halved by the square root; sqrtf and the division
    are correctly rounded, u each.  Per norm <= (d / 2 + 2) u, the two together <= (d + 4) u relative: (d + 4) u |s|.
  * the two multiplications by rn: 2 u |s|.
  Sum: d u (A + |s|) + 6 u |s| <= d u (A + |s|) + 8 u |s| (second-order terms).  bound = 2 * that, doubled for margin.
Checked on the CPU: an fp32 emulation with another summation order stays below 0.04 of this bound at d in {32, 96, 448,
13056} (tests/test_nn_cosine_cpu.py prints the ratios); the worst-case bound itself is about 3e-3 at d = 13056 and 6e-6 at d = 32 (unit-scale random inputs).

Designed inputs (`designed`): every row has exactly 16 entries of +-1 and zeros elsewhere, so ss = 16, rn = 0.25 exactly,
every dot product is an integer and every sim a multiple of 1/16: any fp32 evaluation equals the float64 one bit for bit,
ties included."""
import numpy as np
import torch

U = 2.0 ** -24


def _f64(t) -> np.ndarray:
    return (t.detach().cpu().to(torch.float64) if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)).numpy()


def rnorm(v: np.ndarray) -> np.ndarray:
    return 1.0 / np.maximum(np.sqrt((v * v).sum(-1)), 1e-8)


def similarity(x, y) -> np.ndarray:
    """x [P, tx, d], y [P, ty, d] (any float dtype) -> float64 sim [P, tx, ty], in the definition's association"""
    x, y = _f64(x), _f64(y)
    return (np.einsum("pic,pjc->pij", x, y) * rnorm(x)[:, :, None]) * rnorm(y)[:, None, :]


def nearest(s: np.ndarray):
    """sim [P, tx, ty] -> (row_sim [P, tx], row_idx, col_sim [P, ty], col_idx), ties to the lowest index"""
    ri, ci = s.argmax(2), s.argmax(1)
    return (np.take_along_axis(s, ri[:, :, None], 2)[:, :, 0], ri.astype(np.int32),
            np.take_along_axis(s, ci[:, None, :], 1)[:, 0, :], ci.astype(np.int32))


def bound(x, y, s: np.ndarray) -> np.ndarray:
    """entry-wise bound [P, tx, ty] between the float64 similarity s and an fp32 evaluation of the definition"""
    x, y = _f64(x), _f64(y)
    d = x.shape[-1]
    A = np.einsum("pic,pjc->pij", np.abs(x), np.abs(y)) * rnorm(x)[:, :, None] * rnorm(y)[:, None, :]
    return 2.0 * (d * U * (A + np.abs(s)) + 8.0 * U * np.abs(s))


def designed(P: int, tx: int, ty: int, d: int, seed: int):
    """(x [P, tx, d], y [P, ty, d]) fp32 with exactly 16 entries of +-1 per row at seeded positions.  X and Y are drawn
    differently (Y's positions come from the lower three quarters of the channels only): a row / column swap changes
    the result.  Planted: two rows of X copied to two positions of Y each, and two rows of Y to two rows of X each, where
    the shapes have room -- rows whose maximum (sim = 1) is attained more than once."""
    rng = np.random.default_rng(seed)

    def draw(t, hi):
        a = np.zeros((P, t, d), np.float32)
        for p in range(P):
            for i in range(t):
                pos = rng.choice(hi, 16, replace=False)
                a[p, i, pos] = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
        return a

    x, y = draw(tx, d), draw(ty, max(16, 3 * d // 4))
    for p in range(P):
        if tx >= 5 and ty >= 3:
            y[p, 0] = y[p, ty - 1] = x[p, 1]
            x[p, 0] = x[p, 3] = y[p, 1]
        if tx >= 100 and ty >= 100:
            y[p, 40] = y[p, 97] = x[p, 70]
            x[p, 11] = x[p, 99] = y[p, 64]
    return torch.from_numpy(x), torch.from_numpy(y)


def rows_with_ties(s: np.ndarray) -> int:
    """rows of sim [P, tx, ty] whose maximum is attained at more than one column"""
    return int(((s == s.max(2, keepdims=True)).sum(2) > 1).sum())


def check_near_tie_tolerant(s: np.ndarray, b: np.ndarray, got_sim: np.ndarray, got_idx: np.ndarray, what=""):
    """The rule for random inputs, along the last axis of s [..., t, n] (pass the transposes for the column side):
    |got_sim - s[i, got_idx]| <= b[i, got_idx];  s[i, got_idx] >= max_j s[i, j] - (b[i, got_idx] + b[i, argmax]);  where the
    float64 best-to-second gap exceeds b[i, argmax] + max_j b[i, j], got_idx IS the float64 argmax.  Returns the share of such rows."""
    n = s.shape[-1]
    assert got_idx.min() >= 0 and got_idx.max() < n, what
    gi = got_idx.astype(np.int64)[..., None]
    am = s.argmax(-1)[..., None]
    s_got, b_got = np.take_along_axis(s, gi, -1)[..., 0], np.take_along_axis(b, gi, -1)[..., 0]
    s_max, b_max = np.take_along_axis(s, am, -1)[..., 0], np.take_along_axis(b, am, -1)[..., 0]
    err = np.abs(got_sim.astype(np.float64) - s_got)
    print(f"{what}: max |sim - s| {err.max():.3e}, min slack {(b_got - err).min():.3e}")
    assert (err <= b_got).all(), (what, float(err.max()), float((err - b_got).max()))
    assert (s_got >= s_max - (b_got + b_max)).all(), (what, float((s_max - s_got).max()))
    if n == 1:
        return 1.0
    second = np.partition(s, n - 2, axis=-1)[..., n - 2]
    clear = (s_max - second) > (b_max + b.max(-1))  # no other column can overtake the float64 best within the bounds
    assert (got_idx[clear] == am[..., 0][clear]).all(), what
    return float(clear.mean())
