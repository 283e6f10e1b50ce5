"""PCA of dense descriptor maps on the device: the column mean, the centred covariance and the projection are libvdr.so
kernels (vdr.ops.col_mean / covariance / pca_project, csrc/pca.hip); the d x d eigen-decomposition between them is
torch.linalg.eigh in float64.  pca_colorize is the drop-in of the reference's visualization_utils.pca_colorize.

solver="subspace" (opt-in) replaces eigh by the library's own top-k solver (vdr.ops.sym_topk, csrc/pca_topk.hip) and picks
the smaller side: the d x d covariance when a problem has at least d rows (or is joint), else the t x t Gram matrix
(vdr.ops.gram) followed by the back-projection (vdr.ops.pca_back_project) -- which also admits descriptors wider than 2048
channels, log-binned ones among them."""
from __future__ import annotations

from dataclasses import dataclass

import warnings

import numpy as np
import torch

from . import ops

SOLVERS = ("eigh", "subspace")


class ConvergenceWarning(UserWarning):
    """fit(solver="subspace"): some problems hit max_iter before their residuals met the tolerance and were decomposed by eigh"""


@dataclass
class Pca:
    """A fitted PCA of `problems` problems (one per image, or one for all images when fitted with joint=True).
    mean [problems, d] fp32; components [problems, k, d] fp32, rows of unit length in descending order of explained
    variance, each with its entry of largest magnitude positive (sklearn's svd_flip(u_based_decision=False));
    explained_variance [problems, k] float64 (eigenvalues of the n - 1 covariance); explained_variance_ratio their share
    of the covariance's trace."""
    mean: torch.Tensor
    components: torch.Tensor
    explained_variance: torch.Tensor
    explained_variance_ratio: torch.Tensor
    # not fields: set by fit(solver="subspace").  side: "covariance" | "gram" (None: the eigh route).  scores [P, t, k] fp32,
    # Gram side only: u_j * sqrt(lambda_j (t - 1)) with the component's sign -- the projection of the fitted maps themselves
    # (sklearn's fit_transform), which is all a map wider than 2048 channels can get.  iters / resid: sym_topk's reports.
    side = None
    scores = None
    iters = None
    resid = None

    def transform(self, x: torch.Tensor, scale: bool = False) -> torch.Tensor:
        """x [P, t, d] (or [t, d]) -> [P, t, k] fp32: (x - mean) . components^T, every image with its problem's mean and
        components (the one set when the fit was joint).  scale=True: min-max scaled over a problem's whole block, as the
        reference's _min_max_scale does -- one range for all k components."""
        single = x.dim() == 2
        if single:
            x = x.unsqueeze(0)
        if x.shape[-1] > 2048:
            raise ValueError(f"Pca.transform: the projection kernel stops at d = 2048, got {x.shape[-1]}; the maps the PCA "
                             "was fitted on have their projection in Pca.scores")
        proj, _ = ops.pca_project(x, self.mean, self.components, scale)
        proj = proj.reshape(x.shape[0], x.shape[1], proj.shape[-1])
        return proj[0] if single else proj


def components_from_covariance(cov: torch.Tensor, k: int):
    """cov [problems, d, d] fp32 -> (components [problems, k, d] fp32, explained_variance [problems, k] float64,
    explained_variance_ratio [problems, k] float64): torch.linalg.eigh in float64 on cov's device, the top k eigenvectors in
    descending order, sign-fixed, rounded once to fp32.  ONE batched call -- a loop of single calls costs 17 ms per 768 x 768
    problem, the batched solver 1 - 2 ms.  A single problem goes in as a batch of two copies: on the torch build
    this was written against the solver takes another route for a batch of one, whose vectors differ in the last float64
    bit, while an element of a larger batch came out bitwise the same in every batch tried.  That is an observation about
    the vendor's solver, not a guarantee of this library: only the kernels (mean, covariance, projection) are
    batch-independent by construction."""
    d = cov.shape[-1]
    c = cov.double()
    w, v = torch.linalg.eigh(c if c.shape[0] > 1 else c.expand(2, d, d).contiguous())
    w, v = w[:c.shape[0]], v[:c.shape[0]]
    lam = w.flip(-1)[:, :k]
    vec = v.flip(-1)[:, :, :k].transpose(1, 2)  # [problems, k, d]
    a = vec.abs()
    col = torch.arange(d, device=cov.device)
    first = torch.where(a == a.max(dim=-1, keepdim=True).values, col, d).min(dim=-1).values  # lowest index wins a tie
    sign = torch.sign(torch.gather(vec, 2, first.unsqueeze(-1)))
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    ratio = lam / torch.diagonal(c, dim1=-2, dim2=-1).sum(-1, keepdim=True)
    return (vec * sign).to(torch.float32).contiguous(), lam.contiguous(), ratio


def subspace_side(P: int, t: int, d: int, joint: bool) -> str:
    """The side fit(solver="subspace") decomposes: the d x d covariance when a problem has at least d rows or is joint,
    else the t x t Gram matrix.  A per-image map beyond the covariance kernel's 2048 channels goes to the Gram side even
    with d rows or more (3969 x 2304, say): it is the side that can take it."""
    rows = P * t if joint else t
    return "covariance" if joint or (rows >= d and d <= 2048) else "gram"


def _check_subspace(P: int, t: int, d: int, k: int, joint: bool, side=None) -> str:
    """fit(solver="subspace")'s refusals, before any device work; returns the side"""
    rows = P * t if joint else t
    if k > rows - 1:
        raise ValueError(f"pca.fit: solver='subspace' needs n_components <= rows - 1 = {rows - 1} (a centred map of {rows} rows "
                         f"has rank {rows - 1} at most), got {k}")
    if d % 32:
        raise ValueError(f"pca.fit: d must be a multiple of 32, got {d}")
    if joint and d > 2048:
        raise ValueError(f"pca.fit: a joint PCA takes the covariance side, d <= 2048, got d = {d}")
    if side is None:
        side = subspace_side(P, t, d, joint)
    if side not in ("covariance", "gram") or (joint and side == "gram"):
        raise ValueError(f"pca.fit: side must be 'covariance' or 'gram' (per image only), got {side!r}")
    if side == "gram" and t > 4096:
        raise ValueError(f"pca.fit: the Gram side takes t <= 4096 rows per image, got {t}")
    if side == "covariance" and d > 2048:
        raise ValueError(f"pca.fit: the covariance side takes d <= 2048, got {d}")
    return side


def _sign_fixed(vec: torch.Tensor):
    """vec [P, k, n] -> (vec with its entry of largest magnitude positive, lowest index on a tie; the signs [P, k, 1])"""
    n = vec.shape[-1]
    a = vec.abs()
    col = torch.arange(n, device=vec.device)
    first = torch.where(a == a.max(dim=-1, keepdim=True).values, col, n).min(dim=-1).values
    sign = torch.sign(torch.gather(vec, 2, first.unsqueeze(-1)))
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    return vec * sign, sign


def _fit_subspace(x: torch.Tensor, k: int, joint: bool, side: str, tol: float, max_iter: int) -> Pca:
    t = x.shape[1]
    if side == "covariance":
        mean, mat = ops.covariance(x, None, joint)
    else:
        mean, mat = ops.gram(x, None)
    lam, vec, iters, resid = ops.sym_topk(mat, k, tol, max_iter)
    lam = lam.double()
    bad = torch.nonzero(~(resid <= tol)).flatten()  # the one look at the device: ran into max_iter (or a resid that is not finite)
    if bad.numel():
        warnings.warn(f"pca.fit: {bad.numel()} of {mat.shape[0]} problems did not converge in {max_iter} iterations "
                      f"(residual above {tol:g}); decomposed by eigh instead", ConvergenceWarning, stacklevel=3)
        bvec, blam, _ = components_from_covariance(mat[bad], k)
        vec, lam = vec.clone(), lam.clone()
        vec[bad], lam[bad] = bvec, blam
    ratio = lam / torch.diagonal(mat, dim1=-2, dim2=-1).double().sum(-1, keepdim=True)
    scores = None
    if side == "gram":
        comps = ops.pca_back_project(x, mean, vec, lam.float())
        comps, sign = _sign_fixed(comps)
        scores = (vec * sign * torch.sqrt(lam.clamp_min(0) * (t - 1)).float().unsqueeze(-1)).transpose(1, 2).contiguous()
        vec = comps.contiguous()
    pca = Pca(mean, vec, lam.contiguous(), ratio)
    pca.side, pca.scores, pca.iters, pca.resid = side, scores, iters, resid
    return pca


def fit(x: torch.Tensor, n_components: int = 3, joint: bool = False, solver: str = "eigh", side=None,
        tol: float = ops.TOPK_TOL, max_iter: int = ops.TOPK_MAX_ITER) -> Pca:
    """PCA of descriptor maps x [P, t, d] (or one map [t, d]) bf16 / fp32 on the device: per image, or of all P * t rows
    together with joint=True.  1 <= n_components <= min(8, d, rows).
    solver="eigh" (default): always the exact covariance route (sklearn picks a randomized solver for wide maps): mean and
    covariance on the device, eigh in float64.  d % 32 == 0, d <= 2048.
    solver="subspace": the library's top-k solver on the smaller side (subspace_side; `side` forces one): the covariance
    (d <= 2048) when rows >= d or joint, else the Gram matrix (t <= 4096, any d % 32 == 0) and the back-projection; the Pca
    then carries side, scores (Gram side), iters and resid.  n_components <= rows - 1.  Problems that do not reach `tol`
    within `max_iter` iterations are decomposed by eigh on the same matrix, with one ConvergenceWarning."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise TypeError("pca.fit: x must be a [P, t, d] or [t, d] tensor")
    if solver not in SOLVERS:
        raise ValueError(f"pca.fit: solver must be one of {SOLVERS}, got {solver!r}")
    if x.dim() == 2:
        x = x.unsqueeze(0)
    k = int(n_components)
    rows = x.shape[0] * x.shape[1] if joint else x.shape[1]
    if not 1 <= k <= min(8, x.shape[2], rows):
        raise ValueError(f"pca.fit: n_components must be 1..min(8, d, rows) = 1..{min(8, x.shape[2], rows)}, got {n_components}")
    if solver == "subspace":
        side = _check_subspace(x.shape[0], x.shape[1], x.shape[2], k, joint, side)
        return _fit_subspace(x, k, joint, side, float(tol), int(max_iter))
    mean, cov = ops.covariance(x, None, joint)
    comps, lam, ratio = components_from_covariance(cov, k)
    return Pca(mean, comps, lam, ratio)


def _otsu_threshold(a: torch.Tensor, nbins: int = 256):
    """skimage.filters.threshold_otsu (0.18) of a float map: a histogram of nbins bins over the map's own range (numpy's
    uniform-bin rule), the bin centre that maximises the between-class variance, the first one on a tie; a constant map
    returns its value.  float64 on a's device."""
    v = a.reshape(-1).double()
    lo, hi = v.min(), v.max()
    if bool(lo == hi):
        return v[0]
    edges = torch.linspace(float(lo), float(hi), nbins + 1, dtype=torch.float64, device=v.device)
    idx = ((v - lo) / (hi - lo) * nbins).long().clamp_(0, nbins - 1)
    idx = idx - (v < edges[idx]).long()
    idx = idx + ((v >= edges[(idx + 1).clamp_(max=nbins)]) & (idx != nbins - 1)).long()
    counts = torch.bincount(idx.clamp_(0, nbins - 1), minlength=nbins).double()
    centers = (edges[:-1] + edges[1:]) / 2
    weight1 = torch.cumsum(counts, 0)
    weight2 = torch.cumsum(counts.flip(0), 0).flip(0)
    mean1 = torch.cumsum(counts * centers, 0) / weight1
    mean2 = (torch.cumsum((counts * centers).flip(0), 0) / weight2.flip(0)).flip(0)
    var12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    best = torch.nonzero(var12 == var12.max()).flatten()[0]
    return centers[best]


def _min_max_scale(a: torch.Tensor) -> torch.Tensor:
    """the reference's _min_max_scale: (a - min) / (max - min) over the whole array, unchanged when max == min"""
    lo, hi = a.min(), a.max()
    return (a - lo) / (hi - lo) if bool(hi != lo) else a


def _remove_background(rgb: torch.Tensor) -> torch.Tensor:
    """the remove_bg step of the reference's pca_colorize on one scaled map [..., k]: Otsu cut on channel 0, every channel
    multiplied by the mask (channel 0 > threshold), the result min-max scaled again.  Plain torch on rgb's device."""
    thresh = _otsu_threshold(rgb[..., 0])
    mask = rgb[..., 0].double() > thresh
    return _min_max_scale(rgb * mask.unsqueeze(-1).to(rgb.dtype))


def _colorize_maps(x: torch.Tensor, n_components: int = 3, joint: bool = False, remove_bg: bool = False,
                   solver: str = "eigh") -> torch.Tensor:
    """x [P, t, d] on the device -> [P, t, k] fp32: one fit, one scaled projection (one range per problem), then the
    remove_bg step per problem.  Beyond the projection kernel's 2048 channels (the Gram side of solver="subspace") the
    projection is the fit's own scores, min-max scaled over a problem's block.  Up to 2048 channels the Gram side is
    projected like the covariance side: its scores come from the bf16-rounded centred map the Gram matrix is made of, the
    kernel projects the fp32-centred one."""
    pca = fit(x, n_components, joint, solver)
    if pca.scores is not None and x.shape[-1] > 2048:
        lo = pca.scores.amin(dim=(1, 2), keepdim=True)
        hi = pca.scores.amax(dim=(1, 2), keepdim=True)
        proj = torch.where(hi != lo, (pca.scores - lo) / torch.where(hi != lo, hi - lo, torch.ones_like(hi)), pca.scores)
    else:
        proj, _ = ops.pca_project(x, pca.mean, pca.components, True)  # [problems, R, k]
    if remove_bg:
        proj = torch.stack([_remove_background(p) for p in proj])
    return proj.reshape(x.shape[0], x.shape[1], proj.shape[-1])


def colorize(features, output_shape, remove_bg: bool = False, solver: str = "eigh"):
    """pca_colorize with the solver of vdr.pca.fit as a keyword: solver="subspace" runs the library's top-k solver and also
    takes maps wider than 2048 channels (log-binned descriptors) through the Gram side.  Everything else is pca_colorize's:
    features (n, d) as a numpy array or a tensor -> output_shape + (3,), min-max scaled over the whole [n, 3] array;
    remove_bg=True zeroes everything at or below the Otsu threshold of channel 0 and rescales; n < 3 returns ones."""
    if solver not in SOLVERS:
        raise ValueError(f"pca_colorize: solver must be one of {SOLVERS}, got {solver!r}")
    is_np = not isinstance(features, torch.Tensor)
    f = torch.as_tensor(np.asarray(features)) if is_np else features
    if f.dim() != 2:
        raise ValueError(f"pca_colorize: features must be (n, d), got {tuple(f.shape)}")
    shape = tuple(int(s) for s in output_shape)
    n = f.shape[0]
    if int(np.prod(shape)) != n:
        raise ValueError(f"pca_colorize: output_shape {shape} does not hold {n} rows")
    if n < 3:
        out = torch.ones(shape + (3,), dtype=torch.float32)
        return out.numpy() if is_np else out.to(f.device)
    if solver == "eigh":
        if f.shape[1] % 32 or f.shape[1] > 2048:
            raise ValueError(f"pca_colorize: d must be a multiple of 32, at most 2048, got {f.shape[1]}")
    else:
        _check_subspace(1, n, f.shape[1], 3, False)
    device = f.device if f.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if f.dtype not in (torch.float32, torch.bfloat16):
        f = f.to(torch.float32)
    rgb = _colorize_maps(f.to(device).unsqueeze(0), 3, False, remove_bg, solver)[0].reshape(shape + (3,))
    return rgb.cpu().numpy() if is_np else rgb


def pca_colorize(features, output_shape, remove_bg: bool = False):
    """Drop-in of the reference's visualization_utils.pca_colorize: features (n, d) -- the (h*w, d) map of
    get_dense_descriptor -- as a numpy array or a tensor; returns output_shape + (3,): the first three principal
    components of that one map, min-max scaled over the whole [n, 3] array; remove_bg=True zeroes everything at or below
    the Otsu threshold of channel 0 and rescales.  n < 3 returns ones, as upstream does.  A numpy input gives a float32
    numpy array, a tensor a float32 tensor on the device.  The work runs on the tensor's own device when that is a HIP
    device, else on the current one.  d % 32 == 0 and d <= 2048 (not asked of the n < 3 branch).  The signature is the
    reference's; vdr.pca.colorize is the same function with a solver= keyword."""
    return colorize(features, output_shape, remove_bg, "eigh")
