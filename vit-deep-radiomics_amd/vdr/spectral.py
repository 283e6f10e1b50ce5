"""Spectral object localisation on the thresholded patch-affinity graph of ONE descriptor map: the Fiedler-vector bipartition
of TokenCut and the lowest-degree seed expansion of LOST, on top of two device ops -- vdr.ops.affinity_bits (the graph
B[i, j] = cos(x_i, x_j) > tau, one bit per pair) and vdr.ops.bits_matvec (its product with a few columns).  Everything else is
plain torch on the caller's stream, and host code on the small patch grid.

The generalised eigenproblem is TokenCut's: W = eps + (1 - eps) B, D = diag(W 1), (D - W) y = lambda D y; the second-smallest
pair is wanted.  With M = D^-1/2 W D^-1/2 (symmetric, largest eigenpair 1, D^1/2 1) it is the LARGEST pair (theta, q) of M on
the complement of D^1/2 1: lambda = 1 - theta, y = D^-1/2 q.  `fiedler` runs Lanczos with full re-orthogonalisation on that
complement, all problems in lockstep, vectors and dot products in float64; the only device product is B v (fp32, the fixed
order of include/vdr.h): W v = eps * sum(v) + (1 - eps) * (B v).

Both methods are written from the papers as remembered (Wang et al., TokenCut, CVPR 2022; Simeoni et al., LOST, BMVC 2021);
parity with their code is not pinned.  LOST compares raw dot products with >= 0; here the graph is cosines > 0."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops


def degree(bits: torch.Tensor) -> torch.Tensor:
    """bits [P, t, pitch] int32 (vdr.ops.affinity_bits) -> the row degrees [P, t] int32, exact popcounts"""
    P, t, _ = bits.shape
    return ops.bits_matvec(bits, torch.zeros((P, t), dtype=torch.float32, device=bits.device), degree=True)[1]


def _bits_product(bits: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """B v for v [P, t] float64: the device product, on v rounded once to fp32"""
    return ops.bits_matvec(bits, v.to(torch.float32)).to(torch.float64)


def _top_ritz(alpha: np.ndarray, beta: np.ndarray, m: int):
    """largest eigenpair (theta, s [m]) of the m x m tridiagonal matrix (alpha[:m], beta[:m-1]) and the residual estimate
    |beta[m-1] * s[m-1]| of its Ritz vector"""
    T = np.diag(alpha[:m])
    if m > 1:
        T += np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    w, S = np.linalg.eigh(T)
    return float(w[-1]), S[:, -1], float(abs(beta[m - 1] * S[m - 1, -1]))


def fiedler(bits: torch.Tensor, eps: float = 1e-5, steps: int = 32, tol: float = 1e-6, seed: int = 0, check_every: int = 4,
            product=None):
    """The second-smallest generalised eigenpair of (D - W) y = lambda D y for the graphs bits [P, t, pitch] (t >= 2).
    Returns (vec [P, t] float64 on the device of bits, y = D^-1/2 q scaled to unit Euclidean norm, its entry of largest
    magnitude positive; val [P] float64; resid [P] float64, the Lanczos estimate |beta_m s_m| of ||M q - theta q||; the steps
    taken).  At most `steps` Lanczos steps (never more than t - 1); every check_every steps the P tridiagonal problems are
    solved on the host and the run stops once every residual estimate is <= tol.  The start vector is drawn from
    torch.Generator(seed) on the host: the result is the same from run to run.  A disconnected B still has a connected W
    (eps > 0).  product: a stand-in for the device product (bits, v fp64 [P, t]) -> B v, for tests without a device."""
    if bits.dim() != 3 or bits.shape[1] < 2:
        raise ValueError(f"fiedler: bits must be [P, t, pitch] with t >= 2, got {tuple(bits.shape)}")
    if not 0.0 < float(eps) < 1.0:
        raise ValueError(f"fiedler: eps must lie in (0, 1), got {eps}")
    if int(steps) < 1 or int(check_every) < 1:
        raise ValueError("fiedler: steps and check_every must be positive")
    prod = _bits_product if product is None else product
    eps = float(eps)
    P, t, _ = bits.shape
    dev = bits.device
    ones = torch.ones((P, t), dtype=torch.float64, device=dev)
    deg = prod(bits, ones)                                  # exact: integers below 2^24
    d = eps * t + (1.0 - eps) * deg
    dis = d.rsqrt()
    q0 = d.sqrt()
    q0 = q0 / q0.norm(dim=1, keepdim=True)

    def apply_m(v):
        u = dis * v
        return dis * (eps * u.sum(dim=1, keepdim=True) + (1.0 - eps) * prod(bits, u))

    g = torch.Generator().manual_seed(int(seed))
    w = torch.randn((P, t), dtype=torch.float64, generator=g).to(dev)
    w = w - (w * q0).sum(1, keepdim=True) * q0
    m_max = min(int(steps), t - 1)
    Q = torch.zeros((P, m_max + 1, t), dtype=torch.float64, device=dev)  # Q[:, 0] = q0, Q[:, j + 1] = Lanczos vector j
    Q[:, 0] = q0
    Q[:, 1] = w / w.norm(dim=1, keepdim=True)
    alpha = torch.zeros((P, m_max), dtype=torch.float64, device=dev)
    beta = torch.zeros((P, m_max), dtype=torch.float64, device=dev)
    alive = torch.ones((P,), dtype=torch.bool, device=dev)   # the Krylov space of the problem has not closed yet
    m = 0
    result = None
    while m < m_max:
        q = Q[:, m + 1]
        w = apply_m(q)
        alpha[:, m] = (w * q).sum(1)
        for _ in range(2):  # full re-orthogonalisation, twice: against q0 and every Lanczos vector so far
            basis = Q[:, :m + 2]
            w = w - torch.einsum("pk,pkt->pt", torch.einsum("pkt,pt->pk", basis, w), basis)
        b = w.norm(dim=1)
        alive = alive & (b > 1e-12)
        beta[:, m] = torch.where(alive, b, torch.zeros_like(b))
        m += 1
        if m < m_max:
            Q[:, m + 1] = torch.where(alive.unsqueeze(1), w / b.clamp_min(1e-300).unsqueeze(1), torch.zeros_like(w))
        if m == m_max or m % int(check_every) == 0:
            a_h, b_h = alpha[:, :m].cpu().numpy(), beta[:, :m].cpu().numpy()
            result = []
            for p in range(P):
                closed = np.nonzero(b_h[p] == 0.0)[0]
                mp = int(closed[0]) + 1 if closed.size else m   # the block in front of the first zero beta
                result.append((mp,) + _top_ritz(a_h[p], b_h[p], mp))
            if all(r[3] <= tol for r in result):
                break
    S = torch.zeros((P, m_max), dtype=torch.float64)
    for p, (mp, _, s, _) in enumerate(result):
        S[p, :mp] = torch.from_numpy(s)
    qv = torch.einsum("pk,pkt->pt", S.to(dev), Q[:, 1:])
    vec = dis * qv
    vec = vec / vec.norm(dim=1, keepdim=True)
    top = vec.gather(1, vec.abs().argmax(dim=1, keepdim=True))
    vec = vec * torch.where(top < 0, -1.0, 1.0)
    val = torch.tensor([1.0 - r[1] for r in result], dtype=torch.float64, device=dev)
    resid = torch.tensor([r[3] for r in result], dtype=torch.float64, device=dev)
    return vec, val, resid, m


def seed_component(mask: np.ndarray, seed: int) -> np.ndarray:
    """mask [gh, gw] bool, seed a flat index with mask[seed] set -> the 4-connected component of mask that holds the seed"""
    gh, gw = mask.shape
    out = np.zeros_like(mask, dtype=bool)
    sy, sx = divmod(int(seed), gw)
    if not mask[sy, sx]:
        return out
    out[sy, sx] = True
    stack = [(sy, sx)]
    while stack:
        y, x = stack.pop()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < gh and 0 <= nx < gw and mask[ny, nx] and not out[ny, nx]:
                out[ny, nx] = True
                stack.append((ny, nx))
    return out


def mask_box(mask: np.ndarray) -> "tuple[int, int, int, int]":
    """(y0, x0, y1, x1) of a non-empty bool [gh, gw] mask, inclusive, in patch units"""
    ys, xs = np.nonzero(mask)
    return int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())


def bipartition_rule(eigvec: np.ndarray):
    """TokenCut's rule on one eigenvector [t]: (bipartition [t] bool, seed).  seed = argmax |eigvec| (lowest index on a tie);
    bipartition = eigvec > mean(eigvec), complemented when it does not hold the seed."""
    v = np.asarray(eigvec, dtype=np.float64)
    seed = int(np.argmax(np.abs(v)))
    part = v > v.mean()
    if not part[seed]:
        part = ~part
    return part, seed


def lost_rule(adj_seed: np.ndarray, deg: np.ndarray, k: int):
    """LOST's rule on one graph: deg [t] the degrees, adj_seed(seed) -> bool [t] the seed's row of B.  Returns (seed, set [t]
    bool): seed the lowest degree (lowest index on a tie); the set holds the seed and those of the k lowest-degree patches
    (ties by ascending index) that are adjacent to it."""
    deg = np.asarray(deg)
    order = np.argsort(deg, kind="stable")
    seed = int(order[0])
    low = np.zeros(deg.shape[0], dtype=bool)
    low[order[:max(int(k), 1)]] = True
    s = low & np.asarray(adj_seed(seed), dtype=bool)
    s[seed] = True
    return seed, s


@dataclass
class TokenCut:
    """Result of tokencut for P maps on a gh x gw grid.  eigvec [P, gh, gw] float64, the Fiedler vector; bipartition [P, gh, gw]
    bool, eigvec > mean flipped to hold the seed; seed [P] int64, flat patch index; mask [P, gh, gw] bool, the 4-connected
    component of the bipartition that holds the seed; box [P, 4] int64 (y0, x0, y1, x1), inclusive patch indices; eigval / resid
    [P] float64 and steps, as `fiedler` returns them; bits [P, t, pitch] int32, the graph that was cut.  stride and patch place
    a grid index in the image: pixel_box()."""
    eigvec: torch.Tensor
    bipartition: torch.Tensor
    seed: torch.Tensor
    mask: torch.Tensor
    box: torch.Tensor
    grid: "tuple[int, int]"
    stride: int
    patch: int
    eigval: torch.Tensor
    resid: torch.Tensor
    steps: int
    bits: torch.Tensor

    def pixel_box(self) -> torch.Tensor:
        """[P, 4] float (y0, x0, y1, x1): the centres of the box's corner patches, patch (gy, gx) at gy * stride + patch / 2"""
        return _pixel_box(self)


@dataclass
class Lost:
    """Result of lost for P maps on a gh x gw grid.  degree [P, gh, gw] int32, the row degrees of the graph; expansion
    [P, gh, gw] bool, the seed and those of the k lowest-degree patches adjacent to it; seed [P] int64, the lowest-degree patch;
    mask [P, gh, gw] bool, the 4-connected component of the expansion set that holds the seed; box [P, 4] int64
    (y0, x0, y1, x1), inclusive patch indices; bits [P, t, pitch] int32, the graph (tau = 0 from the model).  pixel_box() as
    TokenCut's."""
    degree: torch.Tensor
    expansion: torch.Tensor
    seed: torch.Tensor
    mask: torch.Tensor
    box: torch.Tensor
    grid: "tuple[int, int]"
    stride: int
    patch: int
    bits: torch.Tensor

    def pixel_box(self) -> torch.Tensor:
        return _pixel_box(self)


def _pixel_box(r) -> torch.Tensor:
    return r.box.to(torch.float32) * r.stride + r.patch / 2


def _masks_and_boxes(parts, seeds, grid, dev):
    """host labelling: (parts [P, gh, gw] bool, seeds [P], masks [P, gh, gw], boxes [P, 4]) as device tensors"""
    gh, gw = grid
    masks = [seed_component(p.reshape(gh, gw), s) for p, s in zip(parts, seeds)]
    boxes = torch.tensor([mask_box(m) for m in masks], dtype=torch.int64, device=dev)
    as_dev = lambda a: torch.from_numpy(np.stack(a)).to(dev).reshape(-1, gh, gw)  # noqa: E731
    return as_dev(parts), torch.tensor(seeds, dtype=torch.int64, device=dev), as_dev(masks), boxes


def check_labelling(what: str, labelling):
    if labelling not in ("host", "device"):
        raise ValueError(f"{what}: labelling must be 'host' or 'device', got {labelling!r}")


def _masks_and_boxes_device(parts, seeds, grid, dev):
    """device labelling: ONE vdr.ops.connected_components call (connectivity 4) labels every map, the seed's component is
    root == root[seed], the box comes from the first and last set row and column; the same tensors as _masks_and_boxes, and
    there is no device-to-host read (the bipartitions and seeds go up as ordinary blocking copies)"""
    from . import components as cc
    gh, gw = grid
    part = torch.from_numpy(np.stack(parts)).to(dev).reshape(-1, gh, gw)
    seed = torch.tensor(seeds, dtype=torch.int64, device=dev)
    root, _, _ = ops.connected_components(part, connectivity=4)
    mask = cc.seed_component(root, seed)
    rows, cols = mask.any(dim=2).to(torch.uint8), mask.any(dim=1).to(torch.uint8)
    first = lambda v: v.argmax(dim=1)                                    # noqa: E731  (the first maximum: the first set row / column)
    last = lambda v: v.shape[1] - 1 - v.flip(1).argmax(dim=1)            # noqa: E731
    return part, seed, mask, torch.stack([first(rows), first(cols), last(rows), last(cols)], dim=1)


def _check_grid(bits, grid, what):
    gh, gw = int(grid[0]), int(grid[1])
    if bits.dim() != 3 or gh <= 0 or gw <= 0 or gh * gw != bits.shape[1]:
        raise ValueError(f"{what}: grid {tuple(grid)} does not have the {bits.shape[1] if bits.dim() == 3 else '?'} patches of bits")
    return gh, gw


def tokencut(bits: torch.Tensor, grid, eps: float = 1e-5, stride: int = 1, patch: int = 1, labelling: str = "host", **fiedler_kwargs) -> TokenCut:
    """TokenCut on the graphs bits [P, t, pitch] of maps on the grid (gh, gw), t = gh * gw: the Fiedler vector (`fiedler`),
    bipartition_rule per map, the seed's 4-connected component, its bounding box.  labelling "host": a numpy flood fill per map;
    "device": one vdr.ops.connected_components call for all maps (the same masks and boxes)."""
    check_labelling("tokencut", labelling)
    gh, gw = _check_grid(bits, grid, "tokencut")
    vec, val, resid, steps = fiedler(bits, eps=eps, **fiedler_kwargs)
    v = vec.cpu().numpy()
    rules = [bipartition_rule(v[p]) for p in range(v.shape[0])]
    label = _masks_and_boxes_device if labelling == "device" else _masks_and_boxes
    parts, seeds, masks, boxes = label([r[0] for r in rules], [r[1] for r in rules], (gh, gw), bits.device)
    return TokenCut(vec.reshape(-1, gh, gw), parts, seeds, masks, boxes, (gh, gw), int(stride), int(patch), val, resid, steps, bits)


def lost(bits: torch.Tensor, grid, k: int = 100, stride: int = 1, patch: int = 1, labelling: str = "host") -> Lost:
    """LOST on the graphs bits [P, t, pitch] (built at tau = 0) of maps on the grid (gh, gw): lost_rule per map, the seed's
    4-connected component of the expansion set, its bounding box.  Host work per call: the degrees come from one bits_matvec
    launch on a zero vector (`degree`: the popcounts ride on the product kernel, there is no kernel of their own), and the seed's
    row of every problem is one small device-to-host copy (pitch words): fine for the tens of maps of a batch, not for thousands.
    labelling as tokencut's."""
    check_labelling("lost", labelling)
    gh, gw = _check_grid(bits, grid, "lost")
    if int(k) < 1:
        raise ValueError(f"lost: k must be positive, got {k}")
    t = gh * gw
    deg = degree(bits)
    deg_h = deg.cpu().numpy()
    seeds, sets = [], []
    for p in range(bits.shape[0]):
        row = lambda s, p=p: ((bits[p, s].cpu().numpy().astype(np.int64)[:, None] >> np.arange(32)) & 1).reshape(-1)[:t] != 0  # noqa: E731
        s, chosen = lost_rule(row, deg_h[p], k)
        seeds.append(s)
        sets.append(chosen)
    label = _masks_and_boxes_device if labelling == "device" else _masks_and_boxes
    parts, seeds, masks, boxes = label(sets, seeds, (gh, gw), bits.device)
    return Lost(deg.reshape(-1, gh, gw), parts, seeds, masks, boxes, (gh, gw), int(stride), int(patch), bits)
