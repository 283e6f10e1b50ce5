"""Float64 restatement of vdr_op_local_correlation's definition (include/vdr.h) and of vdr.local.soft_displacement, with the
bounds between them and any fp32 evaluation, for tests/test_local_correlation_cpu.py, tests/test_local_correlation_gpu.py
and tests/test_propagate_gpu.py.

Definition, for X, Y [t, d] on one gh x gw grid, row i = qy * gw + qx, W = 2 r + 1:
    slot w = (dy + r) * W + (dx + r), dy and dx in [-r, r];  candidate j = (qy + dy) * gw + (qx + dx)
    cost[i, w] = sim(i, j) (nn_cosine_ref.similarity) when (qy + dy, qx + dx) is inside the grid, -inf otherwise
    best_sim[i] = max over the in-grid slots, best_idx[i] the lowest j attaining it (slots ascend with j: numpy's argmax,
    the FIRST maximum, over the slots).
`cost` gathers nn_cosine_ref.similarity to the slots, `bound` gathers nn_cosine_ref.bound (0 at the out-of-grid slots: -inf
is exact); `brute` is the same definition as a triple loop that shares nothing with the gather.

soft_displacement (`soft_displacement`, float64): over the in-grid slots of a cost row, w_s = softmax(cost_s / T),
flow = sum_s w_s * (dy_s, dx_s) in slot order, conf = max_s w_s.  The bound between it and the fp32 evaluation of
vdr.local.soft_displacement FED THE SAME fp32 cost (`soft_bound`), u = 2^-24, n = W * W slots, Z = max_s |cost_s / T| and
A = max_s cost_s / T - min_s cost_s / T over the in-grid slots:
  * z_s = cost_s / T: one fp32 division, |dz_s| <= u |z_s| <= u Z; the largest z is subtracted: the difference of two such
    values and one rounding, |d(z_s - m)| <= 2 u Z + u A.  An absolute error e in the exponent is a relative error e (to first
    order) in exp;
  * exp itself: fp32 library exponentials are good to a few ulp; 4 ulp = 8 u relative is granted;
  * the denominator: a sum of n non-negative terms each with the relative error above, plus (n - 1) u for the fp32 additions
    in any order;  the division: u.
    A weight's relative error: eps_w <= 2 (2 u Z + u A + 8 u) + (n - 1) u + u = u (4 Z + 2 A + 16 + n);
  * flow: each product w_s * o_s is one rounding (u), the sum of n terms in slot order (n - 1) u of sum_s |w_s o_s| <= r:
    |dflow| <= (eps_w + n u) * sum_s w_s |o_s|;   conf: |dconf| <= eps_w * conf.
  Both are doubled for margin, as nn_cosine_ref.bound is."""
import numpy as np

import nn_cosine_ref as nref

U = nref.U


def offsets(r: int) -> np.ndarray:
    """[W * W, 2] int64: the (dy, dx) of every slot"""
    W = 2 * r + 1
    w = np.arange(W * W)
    return np.stack((w // W - r, w % W - r), axis=1).astype(np.int64)


def window(gh: int, gw: int, r: int):
    """(j [t, W * W] int64, the candidate of every (query, slot), 0 where it is outside the grid; ok [t, W * W] bool)"""
    off = offsets(r)
    i = np.arange(gh * gw)
    cy = (i // gw)[:, None] + off[None, :, 0]
    cx = (i % gw)[:, None] + off[None, :, 1]
    ok = (cy >= 0) & (cy < gh) & (cx >= 0) & (cx < gw)
    return np.where(ok, cy * gw + cx, 0), ok


def gather(full: np.ndarray, grid, r: int, fill: float) -> np.ndarray:
    """[P, t, t] -> [P, t, W * W]: entry (i, j) at the slot of j in i's window, `fill` at the out-of-grid slots"""
    j, ok = window(grid[0], grid[1], r)
    return np.where(ok[None], np.take_along_axis(full, np.broadcast_to(j[None], (full.shape[0],) + j.shape), 2), fill)


def cost(x, y, grid, r: int) -> np.ndarray:
    """x, y [P, t, d] -> float64 cost [P, t, W * W]"""
    return gather(nref.similarity(x, y), grid, r, -np.inf)


def bound(x, y, grid, r: int) -> np.ndarray:
    """the entry-wise bound of nn_cosine_ref gathered to the slots, 0 where the slot is outside the grid"""
    return gather(nref.bound(x, y, nref.similarity(x, y)), grid, r, 0.0)


def best(c: np.ndarray, grid, r: int):
    """cost [P, t, W * W] -> (best_sim [P, t] float64, best_idx [P, t] int32, best_slot [P, t] int64)"""
    j, _ = window(grid[0], grid[1], r)
    slot = c.argmax(-1)
    return (np.take_along_axis(c, slot[..., None], -1)[..., 0],
            np.take_along_axis(np.broadcast_to(j[None], c.shape), slot[..., None], -1)[..., 0].astype(np.int32), slot)


def slot_of(idx: np.ndarray, grid, r: int) -> np.ndarray:
    """candidate indices [P, t] -> their slots in the window of query i (every one must be inside it)"""
    gh, gw = grid
    i = np.arange(gh * gw)[None]
    dy, dx = idx // gw - i // gw, idx % gw - i % gw
    assert (np.abs(dy) <= r).all() and (np.abs(dx) <= r).all(), "a candidate outside the window"
    return ((dy + r) * (2 * r + 1) + (dx + r)).astype(np.int64)


def brute(x, y, grid, r: int):
    """the definition as loops: (cost [P, t, W * W] float64, best_sim [P, t], best_idx [P, t] int32)"""
    x, y = nref._f64(x), nref._f64(y)
    gh, gw = grid
    P, t, W = x.shape[0], gh * gw, 2 * r + 1
    rx, ry = nref.rnorm(x), nref.rnorm(y)
    c = np.full((P, t, W * W), -np.inf)
    bs = np.full((P, t), -np.inf)
    bi = np.full((P, t), -1, np.int32)
    for p in range(P):
        for qy in range(gh):
            for qx in range(gw):
                i = qy * gw + qx
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        cy, cx = qy + dy, qx + dx
                        if 0 <= cy < gh and 0 <= cx < gw:
                            j = cy * gw + cx
                            v = (np.dot(x[p, i], y[p, j]) * rx[p, i]) * ry[p, j]
                            c[p, i, (dy + r) * W + dx + r] = v
                            if v > bs[p, i]:  # (j ascends in this loop order: a strict > keeps the lowest)
                                bs[p, i], bi[p, i] = v, j
    return c, bs, bi


def soft_displacement(c, r: int, temperature: float):
    """cost [P, t, W * W] (any float dtype, -inf at the out-of-grid slots) -> float64 (flow [P, t, 2], conf [P, t])"""
    c = nref._f64(c)
    z = c / float(temperature)
    e = np.exp(z - z.max(-1, keepdims=True))  # (exp(-inf) = 0: the out-of-grid slots drop out)
    w = e / e.sum(-1, keepdims=True)
    return w @ offsets(r).astype(np.float64), w.max(-1)


def soft_bound(c, r: int, temperature: float):
    """(flow bound [P, t, 2], conf bound [P, t]) of the module docstring"""
    c = nref._f64(c)
    fin = np.isfinite(c)
    z = c / float(temperature)
    Z = np.where(fin, np.abs(z), 0.0).max(-1)
    A = np.where(fin, z, -np.inf).max(-1) - np.where(fin, z, np.inf).min(-1)
    n = c.shape[-1]
    eps_w = U * (4.0 * Z + 2.0 * A + 16.0 + n)
    e = np.exp(z - z.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    mass = w @ np.abs(offsets(r)).astype(np.float64)
    return 2.0 * (eps_w + n * U)[..., None] * mass, 2.0 * eps_w * w.max(-1)
