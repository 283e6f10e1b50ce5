"""PCA of dense descriptor maps on the device: the column mean, the centred covariance and the projection are libvdr.so
kernels (vdr.ops.col_mean / covariance / pca_project, csrc/pca.hip); the d x d eigen-decomposition between them is
torch.linalg.eigh in float64.  pca_colorize is the drop-in of the reference's visualization_utils.pca_colorize."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops

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

    def transform(self, x: torch.Tensor, scale: bool = False) -> torch.Tensor:
        """x [P, t, d] (or [t, d]) -> [P, t, k] fp32: (x - mean) . components^T, every image with its problem's mean and
        components (the one set when the fit was joint).  scale=True: min-max scaled over a problem's whole block, as the
        reference's _min_max_scale does -- one range for all k components."""
        single = x.dim() == 2
        if single:
            x = x.unsqueeze(0)
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


def fit(x: torch.Tensor, n_components: int = 3, joint: bool = False) -> Pca:
    """PCA of descriptor maps x [P, t, d] (or one map [t, d]) bf16 / fp32 on the device: per image, or of all P * t rows
    together with joint=True.  Always the exact covariance route (sklearn picks a randomized solver for wide maps): mean
    and covariance on the device, eigh in float64.  d % 32 == 0, d <= 2048, 1 <= n_components <= min(8, d, rows)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise TypeError("pca.fit: x must be a [P, t, d] or [t, d] tensor")
    if x.dim() == 2:
        x = x.unsqueeze(0)
    k = int(n_components)
    rows = x.shape[0] * x.shape[1] if joint else x.shape[1]
    if not 1 <= k <= min(8, x.shape[2], rows):
        raise ValueError(f"pca.fit: n_components must be 1..min(8, d, rows) = 1..{min(8, x.shape[2], rows)}, got {n_components}")
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


def _colorize_maps(x: torch.Tensor, n_components: int = 3, joint: bool = False, remove_bg: bool = False) -> torch.Tensor:
    """x [P, t, d] on the device -> [P, t, k] fp32: one fit, one scaled projection (one range per problem), then the
    remove_bg step per problem."""
    pca = fit(x, n_components, joint)
    proj, _ = ops.pca_project(x, pca.mean, pca.components, True)  # [problems, R, k]
    if remove_bg:
        proj = torch.stack([_remove_background(p) for p in proj])
    return proj.reshape(x.shape[0], x.shape[1], proj.shape[-1])


def pca_colorize(features, output_shape, remove_bg: bool = False):
    """Drop-in of the reference's visualization_utils.pca_colorize: features (n, d) -- the (h*w, d) map of
    get_dense_descriptor -- as a numpy array or a tensor; returns output_shape + (3,): the first three principal
    components of that one map, min-max scaled over the whole [n, 3] array; remove_bg=True zeroes everything at or below
    the Otsu threshold of channel 0 and rescales.  n < 3 returns ones, as upstream does.  A numpy input gives a float32
    numpy array, a tensor a float32 tensor on the device.  The work runs on the tensor's own device when that is a HIP
    device, else on the current one.  d % 32 == 0 and d <= 2048 (not asked of the n < 3 branch)."""
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
    if f.shape[1] % 32 or f.shape[1] > 2048:
        raise ValueError(f"pca_colorize: d must be a multiple of 32, at most 2048, got {f.shape[1]}")
    device = f.device if f.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if f.dtype not in (torch.float32, torch.bfloat16):
        f = f.to(torch.float32)
    rgb = _colorize_maps(f.to(device).unsqueeze(0), 3, False, remove_bg)[0].reshape(shape + (3,))
    return rgb.cpu().numpy() if is_np else rgb
