"""float64 restatement of the three definitions of include/vdr.h behind vdr.pca.fit(solver="subspace") -- vdr_op_gram,
vdr_op_sym_topk, vdr_op_pca_back_project --, the planted-spectrum matrices the solver is tested on, and the composition
(fit on either side).  CPU only; numpy and torch.

The steps the definitions fix in a narrower format are kept: the centring float(x) - mean is one fp32 subtraction rounded
once to bf16 (gram), the solver's blocks V, W and Z are rounded to fp32 where the device stores them.  Everything else is
float64, so this is the definition without its fp32 summation error, not a bit-for-bit model."""
import numpy as np
import torch

import pca_ref as pref

GRAM_CHUNK = 256   # VDR_GRAM_CHUNK
TOPK_SLAB = 128    # VDR_TOPK_SLAB
BLOCK = 16
SWEEPS = 10
U = pref.U


# ---- gram / back-projection -------------------------------------------------------------------------------------------
def gram(x: torch.Tensor, mean: torch.Tensor):
    """x [t, d], mean [d] -> (gram float64 [t, t], bound [t, t]): z z^T / (t - 1); the products are exact in fp32, the error is
    that of summing d terms in fp32 (any order: gamma_d) and of one division."""
    z = pref.centred_bf16(x, mean)
    t, d = x.shape
    g = z @ z.t() / (t - 1)
    bound = pref.gamma(d) * (z.abs() @ z.abs().t()) / (t - 1) + U * g.abs() + 1e-45
    return g, bound


def back_project(x: torch.Tensor, mean: torch.Tensor, u: torch.Tensor, values: torch.Tensor):
    """x [t, d], mean [d], u [k, t], values [k] -> (components float64 [k, d] of unit length, raw float64 [k, d], bound on raw):
    raw[j] = sum_r u[j, r] * fl(float(x[r]) - mean); each product rounded once, t terms summed in fp32: gamma_{t+1}."""
    v = (pref.f32(x) - pref.f32(mean)).double()
    w = pref.f32(u).double()
    raw = w @ v
    bound = pref.gamma(x.shape[0] + 1) * (w.abs() @ v.abs()) + 1e-45
    norm = raw.norm(dim=1, keepdim=True)
    live = (pref.f32(values).double().reshape(-1, 1) > 0) & (norm > 0)
    comps = torch.where(live, raw / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(raw))
    return comps, raw, bound


# ---- the solver -------------------------------------------------------------------------------------------------------
def start_hash(rows: int, cols: int) -> np.ndarray:
    """the +-1 pattern of the start block: bit 0 of an integer hash of (row, column), uint32 arithmetic"""
    r = np.arange(rows, dtype=np.uint64).reshape(-1, 1)
    c = np.arange(cols, dtype=np.uint64).reshape(1, -1)
    m = np.uint64(0xFFFFFFFF)
    h = ((r * np.uint64(0x9E3779B1)) & m) ^ ((c * np.uint64(0x85EBCA6B)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return np.where(h & np.uint64(1), -1.0, 1.0)


def start_block(n: int) -> np.ndarray:
    """[n, 16] before orthonormalisation: the identity for n <= 16, else the hash pattern; columns >= min(16, n) zero"""
    z = np.zeros((n, BLOCK))
    b = min(BLOCK, n)
    z[:, :b] = np.eye(n)[:, :b] if n <= BLOCK else start_hash(n, b)
    return z


def partner(i: int, step: int) -> int:
    if i == 15:
        return step
    if i == step:
        return 15
    return (2 * step - i + 30) % 15


def jacobi16(h: np.ndarray):
    """cyclic Jacobi of a symmetric 16 x 16 float64 matrix in round-robin order, 8 disjoint rotations at a time, until a
    sweep leaves no off-diagonal entry above 2^-52 of the largest diagonal one, SWEEPS sweeps at most -> (diag, Y): H_end = Y^T H Y"""
    h = h.copy()
    y = np.eye(BLOCK)
    for _ in range(SWEEPS):
        off = np.abs(h - np.diag(np.diag(h))).max()
        if off <= np.abs(np.diag(h)).max() * 2.0 ** -52:
            break
        for step in range(15):
            j = np.eye(BLOCK)
            for i in range(BLOCK):
                q = partner(i, step)
                if i > q:
                    continue
                apq, app, aqq = h[i, q], h[i, i], h[q, q]
                if abs(apq) > 1e-300 and abs(apq) > 1e-40 * (abs(app) + abs(aqq)):
                    tau = (aqq - app) / (2.0 * apq)
                    tt = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                    c = 1.0 / np.sqrt(1.0 + tt * tt)
                    s = tt * c
                    j[i, i] = j[q, q] = c
                    j[i, q], j[q, i] = s, -s
            h = j.T @ h @ j
            y = y @ j
    return np.diag(h).copy(), y


def orthonormalise(z: np.ndarray) -> np.ndarray:
    """z [n, 16] (fp32 values) -> V [n, 16] fp32 values: Cholesky of G = z^T z, V = z L^-T; a column whose pivot is not above
    2^-30 of its diagonal is dropped (zero)"""
    g = z.T @ z
    g = 0.5 * (g + g.T)
    L = np.zeros((BLOCK, BLOCK))
    live = np.zeros(BLOCK, bool)
    for c in range(BLOCK):
        d = g[c, c] - (L[c, :c] ** 2).sum()
        live[c] = g[c, c] > 0 and d > g[c, c] * 2.0 ** -30
        if live[c]:
            L[c, c] = np.sqrt(d)
            for i in range(c + 1, BLOCK):
                L[i, c] = (g[i, c] - (L[i, :c] * L[c, :c]).sum()) / L[c, c]
    x = np.zeros_like(z)
    for c in range(BLOCK):
        if live[c]:
            x[:, c] = (z[:, c] - x[:, :c] @ L[c, :c]) / L[c, c]
    return x.astype(np.float32).astype(np.float64)


def sign_fix(v: np.ndarray) -> np.ndarray:
    """rows of v: the entry of largest magnitude positive, lowest index on a tie"""
    out = v.copy()
    for j in range(v.shape[0]):
        at = int(np.argmax(np.abs(v[j])))  # (argmax returns the first maximum)
        if v[j, at] < 0:
            out[j] = -v[j]
    return out


def sym_topk(a: np.ndarray, k: int, tol: float, max_iter: int):
    """a [n, n] fp32 values -> (values [k], vectors [k, n], iters, resid), the definition of vdr_op_sym_topk"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    n = a.shape[0]
    v = orthonormalise(start_block(n))
    for it in range(max_iter):
        w = (a.T @ v).astype(np.float32).astype(np.float64)
        h = v.T @ w
        theta, y = jacobi16(0.5 * (h + h.T))
        order = sorted(range(BLOCK), key=lambda q: (-theta[q], q))
        th = theta[order]
        vy, wy = v @ y[:, order], w @ y[:, order]
        res = np.linalg.norm(wy - th * vy, axis=0)
        worst = res[:k].max()
        if worst <= np.float32(tol).astype(np.float64) * th[0] or it + 1 >= max_iter:
            norm = np.linalg.norm(vy[:, :k], axis=0)
            vec = np.where(norm > 0, vy[:, :k] / np.where(norm > 0, norm, 1.0), 0.0).T.astype(np.float32)
            return th[:k].astype(np.float32), sign_fix(vec), it + 1, float(worst / th[0]) if th[0] > 0 else 0.0
        live = (th > 0) & (th > th[0] * 2.0 ** -40)
        z = np.where(live, wy / np.where(live, th, 1.0), 0.0).astype(np.float32).astype(np.float64)
        v = orthonormalise(z)
    raise AssertionError("unreachable")


# ---- planted spectra --------------------------------------------------------------------------------------------------------
def planted(n: int, lam, seed: int):
    """A = Q diag(lam) Q^T in float64 with a random orthogonal Q, rounded once to fp32, symmetrised -> (A fp32 [n, n],
    Q float64 [n, n] with the eigenvectors in its columns, lam float64 [n])"""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    q = q * np.sign(np.diag(r))
    lam = np.asarray(lam, dtype=np.float64)
    a = (q * lam) @ q.T
    a = a.astype(np.float32)
    a = np.triu(a) + np.triu(a, 1).T
    return a, q, lam


def sine(x, v) -> float:
    """sine of the angle between x and the unit vector v, from the part of x orthogonal to v (1 - cos^2 cancels)"""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return float(np.linalg.norm(x - (x @ v) * v) / np.linalg.norm(x))


def geometric(n: int, ratio: float, floor: float = 1e-6) -> np.ndarray:
    """lam_j = max(ratio^j, floor)"""
    return np.maximum(ratio ** np.arange(n, dtype=np.float64), floor)


# ---- the composition -----------------------------------------------------------------------------------------------------------
def fit(x: torch.Tensor, k: int, side: str, tol: float, max_iter: int):
    """fit(solver="subspace") on one map x [t, d] through this restatement
    -> (mean fp32 [d], components fp32 [k, d], explained_variance float64 [k], ratio float64 [k], scores float64 [t, k] or None)"""
    mean = pref.col_mean(x)[0].float()
    t = x.shape[0]
    if side == "covariance":
        mat = pref.covariance(x, mean)[0].float().numpy()
        lam, vec, _, _ = sym_topk(mat, k, tol, max_iter)
        return mean, torch.from_numpy(vec), torch.from_numpy(lam.astype(np.float64)), \
            torch.from_numpy(lam.astype(np.float64) / np.trace(mat.astype(np.float64))), None
    mat = gram(x, mean)[0].float().numpy()
    lam, u, _, _ = sym_topk(mat, k, tol, max_iter)
    comps = back_project(x, mean, torch.from_numpy(u), torch.from_numpy(lam))[0].float().numpy()
    fixed = sign_fix(comps)
    sign = np.where((fixed * comps).sum(1) < 0, -1.0, 1.0)
    lam64 = lam.astype(np.float64)
    scores = (u.astype(np.float64) * sign[:, None] * np.sqrt(np.maximum(lam64, 0) * (t - 1))[:, None]).T
    return mean, torch.from_numpy(fixed), torch.from_numpy(lam64), torch.from_numpy(lam64 / np.trace(mat.astype(np.float64))), scores
