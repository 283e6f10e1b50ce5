"""Anomaly maps of dense descriptors by the Gaussian-of-features family: one multivariate Gaussian over all patch
descriptors (Rippel et al.), one Gaussian per patch position (PaDiM), and a memory bank (PatchCore's cheap sibling).  The
fit is vdr.ops.covariance plus one float64 eigen-decomposition in torch; the score is ONE kernel, vdr.ops.mahalanobis
(csrc/mahalanobis.hip), which never writes the whitened [rows, k] matrix.  Everything else here is plain torch.

Deviations, stated: the shrinkage is a given constant (sklearn's ShrunkCovariance), not Ledoit-Wolf / OAS; PaDiM's random
channel subset is replaced by n_components (the leading whitened directions); PatchCore's k-NN re-weighting of the image
score is absent (it needs a top-k kernel); parity with anomalib's code is not pinned; a fit is at most 2048 channels wide
(vdr.ops.covariance)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops


def whitening(cov: torch.Tensor, n: int, shrinkage: float = 0.0, ridge: float = 0.0, n_components=None):
    """Whitening rows of covariance matrices: cov [P, d, d] (fp32 or float64) with the n - 1 divisor of vdr.ops.covariance,
    fitted on n rows -> (whiten [P, k, d] fp32, eigenvalues [P, k] float64, descending).  The covariance is converted to
    sklearn's 1 / n form S = cov (n - 1) / n, shrunk by ShrunkCovariance's rule (1 - shrinkage) S + shrinkage tr(S) / d I, and
    ridge * I is added (PaDiM: 0.01); one batched float64 torch.linalg.eigh on cov's device; W = Lambda^-1/2 V^T, so that
    sum_j (W (x - mu))_j^2 is the squared Mahalanobis distance; n_components keeps the rows of the largest eigenvalues; one
    rounding to fp32.  A non-positive eigenvalue is refused."""
    if not isinstance(cov, torch.Tensor) or cov.dim() != 3 or cov.shape[1] != cov.shape[2] or \
            cov.dtype not in (torch.float32, torch.float64):
        raise TypeError("whitening: cov must be a [P, d, d] float32 or float64 tensor")
    if isinstance(n, bool) or int(n) < 2:
        raise ValueError(f"whitening: n must be at least 2 rows, got {n!r}")
    if not 0.0 <= float(shrinkage) <= 1.0 or not float(ridge) >= 0.0:
        raise ValueError(f"whitening: shrinkage must be in 0..1 and ridge >= 0, got {shrinkage} and {ridge}")
    d = int(cov.shape[1])
    k = d if n_components is None else int(n_components)
    if not 1 <= k <= d:
        raise ValueError(f"whitening: n_components must be 1..{d}, got {n_components!r}")
    n = int(n)
    s = cov.to(torch.float64) * ((n - 1) / n)
    eye = torch.eye(d, dtype=torch.float64, device=cov.device)
    tr = s.diagonal(dim1=1, dim2=2).sum(-1)
    s = (1.0 - float(shrinkage)) * s + (float(shrinkage) * tr / d).view(-1, 1, 1) * eye + float(ridge) * eye
    vals, vecs = torch.linalg.eigh(s)  # ascending
    vals, vecs = vals.flip(-1)[:, :k], vecs.flip(-1)[:, :, :k]
    if not bool((vals > 0).all()):
        raise ValueError(f"whitening: the covariance has a non-positive eigenvalue ({float(vals.min()):.3e}): it is singular "
                         "to working precision; raise `shrinkage` or `ridge`, or keep fewer n_components")
    w = vecs.transpose(1, 2) * vals.rsqrt().unsqueeze(-1)
    return w.to(torch.float32).contiguous(), vals


@dataclass
class Gaussian:
    """A fitted Gaussian model of descriptors.  Global (per_position False): mean [1, d], whiten [1, k, d]; per position
    (PaDiM): mean [t, d], whiten [t, k, d], position p of a map is problem p.  eigenvalues [P, k] float64 descending (of the
    shrunk 1 / n covariance); n: the rows behind every Gaussian; grid: the (gh, gw) patch grid of the fit when known."""
    mean: torch.Tensor
    whiten: torch.Tensor
    eigenvalues: torch.Tensor
    n: int
    per_position: bool
    grid: object = None

    def score(self, x: torch.Tensor) -> torch.Tensor:
        """Squared Mahalanobis distance of every row: x [B, t, d] bf16 / fp32 on the device (views with contiguous channels are
        read in place) -> [B, t] fp32.  One vdr.ops.mahalanobis call: a global model enters with problem stride 0 under the
        B maps; a per-position model takes the map as [t, B, 1, d], position p under Gaussian p."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise TypeError("Gaussian.score: x must be a [B, t, d] float32 or bfloat16 tensor")
        B, t, d = x.shape
        P, k = int(self.whiten.shape[0]), int(self.whiten.shape[1])
        if d != self.mean.shape[1]:
            raise ValueError(f"Gaussian.score: the model has {self.mean.shape[1]} channels, x has {d}")
        if not self.per_position:
            return ops.mahalanobis(x, self.mean.expand(B, d), self.whiten.expand(B, k, d))
        if t != P:
            raise ValueError(f"Gaussian.score: a per-position model of {P} positions cannot score maps of {t} rows")
        return ops.mahalanobis(x.transpose(0, 1).unsqueeze(2), self.mean, self.whiten).t().contiguous()


class GaussianAccumulator:
    """Mean and covariance of descriptor rows over any number of batches.  add(x [B, t, d]) is one vdr.ops.covariance call:
    all B * t rows as one problem (joint), or with per_position=True the batch viewed as [t, B, d] -- position p is problem p,
    no copy.  Batches are merged in float64 by the pairwise rule of Chan et al.:
    M2 = M2a + M2b + delta delta^T na nb / n, mean = mean_a + delta nb / n."""

    def __init__(self, per_position: bool = False):
        self.per_position = bool(per_position)
        self.n = 0
        self.mean = None  # [P, d] float64
        self.m2 = None    # [P, d, d] float64
        self.grid = None

    def add(self, x: torch.Tensor) -> "GaussianAccumulator":
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise TypeError("GaussianAccumulator.add: x must be a [B, t, d] float32 or bfloat16 tensor")
        B, t, d = x.shape
        if self.mean is not None and (d != self.mean.shape[1] or (self.per_position and t != self.mean.shape[0])):
            raise ValueError(f"GaussianAccumulator.add: a batch of shape {tuple(x.shape)} after batches of "
                             f"{self.mean.shape[0] if self.per_position else 'any'} positions and {self.mean.shape[1]} channels")
        if self.per_position:
            if B < 2:
                raise ValueError("GaussianAccumulator.add: a per-position batch needs at least 2 images")
            mean, cov = ops.covariance(x.transpose(0, 1))
            nb = B
        else:
            mean, cov = ops.covariance(x, joint=True)
            nb = B * t
        return self.merge(nb, mean.to(torch.float64), cov.to(torch.float64) * (nb - 1))

    def merge(self, nb: int, mean: torch.Tensor, m2: torch.Tensor) -> "GaussianAccumulator":
        """the moments of one more batch -- nb rows, mean [P, d], m2 [P, d, d] = the sum of the centred outer products, both
        float64 -- merged by the pairwise rule"""
        if self.mean is None:
            self.n, self.mean, self.m2 = int(nb), mean, m2
            return self
        na, n = self.n, self.n + int(nb)
        delta = mean - self.mean
        self.m2 = self.m2 + m2 + delta.unsqueeze(2) * delta.unsqueeze(1) * (na * nb / n)
        self.mean = self.mean + delta * (nb / n)
        self.n = n
        return self

    def covariance(self) -> torch.Tensor:
        """the merged covariance [P, d, d] float64 with the n - 1 divisor"""
        if self.mean is None:
            raise ValueError("GaussianAccumulator: no batch was added")
        return self.m2 / (self.n - 1)

    def finish(self, shrinkage: float = 0.0, ridge: float = 0.0, n_components=None) -> Gaussian:
        w, vals = whitening(self.covariance(), self.n, shrinkage, ridge, n_components)
        return Gaussian(self.mean.to(torch.float32).contiguous(), w, vals, self.n, self.per_position, self.grid)


def fit_gaussian(x: torch.Tensor, per_position: bool = False, shrinkage: float = 0.0, ridge: float = 0.0,
                 n_components=None) -> Gaussian:
    """GaussianAccumulator(per_position).add(x).finish(...): the one-batch form"""
    return GaussianAccumulator(per_position).add(x).finish(shrinkage, ridge, n_components)


class MemoryBank:
    """A bank of m normal descriptors [m, d] (kept in bf16); score(x [B, t, d]) -> [B, t] fp32 = 1 - the cosine to the
    nearest bank row, by vdr.ops.nn_cosine with the bank under every map at stride 0.  score(x, k) with k > 1: the mean of the
    k smallest distances 1 - cos (vdr.ops.knn), added nearest first and divided once.  reweight=True is PatchCore's
    re-weighting of the nearest distance d_1 by the neighbourhood: (1 - softmax(d)[0]) * d_1 over the k distances d (k >= 2),
    which lowers the score of a patch whose nearest bank rows are all about equally far."""

    def __init__(self, bank: torch.Tensor):
        if not isinstance(bank, torch.Tensor) or bank.dim() != 2 or bank.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("MemoryBank: bank must be a [m, d] float32 or bfloat16 tensor")
        self.bank = bank.to(torch.bfloat16).contiguous()

    def score(self, x: torch.Tensor, k: int = 1, reweight: bool = False) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise TypeError("MemoryBank.score: x must be a [B, t, d] float32 or bfloat16 tensor")
        m, d = self.bank.shape
        bank = self.bank.unsqueeze(0).expand(x.shape[0], m, d)
        if isinstance(k, bool) or int(k) != k or int(k) < 1:
            raise ValueError(f"MemoryBank.score: k must be a positive integer, got {k!r}")
        if reweight and int(k) < 2:
            raise ValueError("MemoryBank.score: reweight=True needs k >= 2")
        if int(k) == 1:
            return 1.0 - ops.nn_cosine(x, bank, mutual=False)[0]
        dist = 1.0 - ops.knn(x, bank, int(k))[0]  # [B, t, k], nearest first
        if reweight:
            return (1.0 - torch.softmax(dist, dim=-1)[..., 0]) * dist[..., 0]
        total = dist[..., 0]
        for j in range(1, int(k)):
            total = total + dist[..., j]
        return total / float(int(k))

    @classmethod
    def coreset(cls, x: torch.Tensor, m: int) -> "MemoryBank":
        """the m rows of x ([B, t, d] or [R, d]) that vdr.kmeans.maximin picks: the deterministic farthest-point coreset"""
        from . import kmeans
        if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
            raise TypeError("MemoryBank.coreset: x must be a [B, t, d] or [R, d] tensor")
        rows = x.reshape(1, -1, x.shape[-1])
        if isinstance(m, bool) or not 1 <= int(m) <= rows.shape[1]:
            raise ValueError(f"MemoryBank.coreset: m must be 1..{rows.shape[1]}, got {m!r}")
        return cls(rows[0][kmeans.maximin(rows, int(m))[0]])


def gaussian_blur(a: torch.Tensor, sigma: float) -> torch.Tensor:
    """a [B, H, W] blurred by a separable Gaussian of `sigma` pixels (radius int(4 sigma + 0.5), border pixels replicated)"""
    r = int(4.0 * float(sigma) + 0.5)
    if r < 1:
        return a
    g = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=a.dtype, device=a.device) / float(sigma)) ** 2)
    g = g / g.sum()
    F = torch.nn.functional
    a = a.unsqueeze(1)
    a = F.conv2d(F.pad(a, (0, 0, r, r), mode="replicate"), g.view(1, 1, -1, 1))
    a = F.conv2d(F.pad(a, (r, r, 0, 0), mode="replicate"), g.view(1, 1, 1, -1))
    return a.squeeze(1)


@dataclass
class AnomalyMap:
    """d2 [B, gh, gw] fp32: the squared Mahalanobis distance of every patch; score [B]: its maximum per image."""
    d2: torch.Tensor

    @property
    def score(self) -> torch.Tensor:
        return self.d2.flatten(1).amax(dim=1)

    def upsample(self, size, sigma: float = 0.0) -> torch.Tensor:
        """the map at `size` = (H, W) pixels: bilinear F.interpolate (align_corners False), then a Gaussian blur of `sigma`
        pixels when sigma > 0 (PaDiM: 4)"""
        up = torch.nn.functional.interpolate(self.d2.unsqueeze(1), size=tuple(size), mode="bilinear", align_corners=False).squeeze(1)
        return gaussian_blur(up, sigma) if sigma > 0 else up

    def upsample_guided(self, x: torch.Tensor, box=None, patch=None, stride=None, radius: int = 2, sigma_spatial: float = 1.0,
                        sigma_range: float = 0.1) -> torch.Tensor:
        """the map at the pixels of `box` = (y0, x0, y1, x1) of the images x [B, Cg, H, W] the map was computed from (None: the
        whole image), by joint bilateral upsampling guided by x (vdr.upsample.guided): [B, h, w] fp32 whose edges follow the
        image's instead of the patch borders.  patch / stride: the grid's geometry; None takes non-overlapping patches of
        H // gh pixels.  The filter is linear in the map, so d2 enters as three bf16 channels hi + mid + lo (24 significant
        bits: nothing of the fp32 distances is lost to the op's bf16 operand) that are added up again."""
        from . import upsample
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[0] != self.d2.shape[0]:
            raise ValueError(f"upsample_guided: x must be the [B, Cg, H, W] images of the map, B = {self.d2.shape[0]}")
        gh, gw = int(self.d2.shape[1]), int(self.d2.shape[2])
        if patch is None:
            if x.shape[2] % gh or x.shape[3] % gw or x.shape[2] // gh != x.shape[3] // gw:
                raise ValueError(f"upsample_guided: a {x.shape[2]} x {x.shape[3]} image over a {gh} x {gw} grid of overlapping or "
                                 "non-square patches needs patch and stride")
            patch = x.shape[2] // gh
        stride = patch if stride is None else stride
        d2 = self.d2.float()
        hi = d2.to(torch.bfloat16).float()
        mid = (d2 - hi).to(torch.bfloat16).float()
        lo = (d2 - hi - mid).to(torch.bfloat16).float()
        up = upsample.guided(torch.stack((hi, mid, lo), dim=-1), x.to(d2.device), patch, stride, radius=radius,
                             sigma_spatial=sigma_spatial, sigma_range=sigma_range, box=box, out_dtype=torch.float32)
        return up[..., 0] + up[..., 1] + up[..., 2]
