"""Overlap and surface-distance measures between two masks, on top of the distance transform (vdr.morphology; the kernel is
csrc/edt.hip).  Plain torch in float64, per plane: masks are [P, H, W] or [H, W] on either device (a volume is compared slice by
slice), results are float64 / int64 tensors [P] on the masks' device.

The SURFACE of a mask is vdr.morphology.boundary: its set pixels with a clear 4-neighbour or on the plane's edge (medpy's
mask ^ binary_erosion(mask)).  The distance from a surface pixel of a to the surface of b is spacing * sqrt(float64(d2)), d2 the
exact squared distance to the nearest surface pixel of b (the transform of the complement of boundary(b)); it runs both ways.

Empty masks: two empty masks are a perfect match (dice = iou = nsd = 1, hd = hd95 = assd = 0).  ONE empty mask against a
non-empty one has no surface to measure to: hd = hd95 = assd = +inf and nsd = 0 (dice = iou = 0).

Parity with medpy, MONAI and DeepMind's surface-distance package is unpinned (none of them was at hand): the rules are restated
on scipy in the tests.  Out of scope: 3-D surfaces and anisotropic spacing (spacing is one scalar)."""
from __future__ import annotations

import math

import torch

from . import components as cc
from . import morphology as mo


def _pair(a, b, what):
    ma, single = cc.as_planes(a, what)
    mb, _ = cc.as_planes(b, what)
    if ma.shape != mb.shape or ma.device != mb.device:
        raise ValueError(f"{what}: the two masks must have one shape and one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    return ma != 0, mb != 0


def overlap(a: torch.Tensor, b: torch.Tensor) -> dict:
    """dice = 2 |a & b| / (|a| + |b|), iou = |a & b| / |a | b| (float64 [P]; 1 for two empty masks) and the three integer counts
    intersection, a and b (int64 [P]).  No synchronisation."""
    ma, mb = _pair(a, b, "overlap")
    P = ma.shape[0]
    inter = (ma & mb).reshape(P, -1).sum(dim=1)
    na, nb = ma.reshape(P, -1).sum(dim=1), mb.reshape(P, -1).sum(dim=1)
    both, union = na + nb, na + nb - inter
    one = torch.ones((), dtype=torch.float64, device=ma.device)
    dice = torch.where(both > 0, 2.0 * inter.to(torch.float64) / both.clamp_min(1).to(torch.float64), one)
    iou = torch.where(union > 0, inter.to(torch.float64) / union.clamp_min(1).to(torch.float64), one)
    return {"dice": dice, "iou": iou, "intersection": inter, "a": na, "b": nb}


def percentile(values: torch.Tensor, q: float) -> torch.Tensor:
    """np.percentile(values, q) with linear interpolation (medpy's rule for hd95): the sorted values at the virtual index
    (n - 1) q / 100, lo + (hi - lo) * fraction"""
    s = torch.sort(values.to(torch.float64)).values
    pos = (s.numel() - 1) * (q / 100.0)
    lo = int(math.floor(pos))
    hi = min(lo + 1, s.numel() - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


def surface(a: torch.Tensor, b: torch.Tensor, spacing: float = 1.0, tolerance: float = 1.0) -> dict:
    """Surface distances between a and b, both ways, per plane (float64 [P]):
      hd    the larger of the two one-way maxima (the Hausdorff distance)
      hd95  the 95th percentile of the two one-way distance sets taken together, linear interpolation (medpy's hd95)
      assd  the mean of the two one-way means (the average symmetric surface distance)
      nsd   the share of the pixels of both surfaces that lie within `tolerance` of the other surface (surface Dice)
    spacing is the pixel size (one scalar), tolerance is in the same unit.  Two empty masks: 0, 0, 0, 1; one empty mask: inf, inf,
    inf, 0.  The surfaces have data-dependent sizes: this function synchronises once per plane."""
    ma, mb = _pair(a, b, "surface")
    if not (isinstance(spacing, (int, float)) and not isinstance(spacing, bool) and spacing > 0 and math.isfinite(spacing)):
        raise ValueError(f"surface: spacing must be a finite number > 0, got {spacing!r}")
    if not (isinstance(tolerance, (int, float)) and not isinstance(tolerance, bool) and tolerance >= 0):
        raise ValueError(f"surface: tolerance must be a number >= 0, got {tolerance!r}")
    P = ma.shape[0]
    sa, sb = mo.boundary(ma), mo.boundary(mb)
    to_a, to_b = mo._edt(sa, 0, False), mo._edt(sb, 0, False)         # the squared distance of every pixel to the surface of a / of b
    out = {k: torch.empty((P,), dtype=torch.float64, device=ma.device) for k in ("hd", "hd95", "assd", "nsd")}
    for p in range(P):
        ab = float(spacing) * to_b[p][sa[p]].to(torch.float64).sqrt()
        ba = float(spacing) * to_a[p][sb[p]].to(torch.float64).sqrt()
        if ab.numel() == 0 and ba.numel() == 0:
            vals = (0.0, 0.0, 0.0, 1.0)
        elif ab.numel() == 0 or ba.numel() == 0:
            vals = (math.inf, math.inf, math.inf, 0.0)
        else:
            both = torch.cat([ab, ba])
            vals = (torch.maximum(ab.max(), ba.max()), percentile(both, 95.0), (ab.mean() + ba.mean()) / 2.0,
                    ((ab <= tolerance).sum() + (ba <= tolerance).sum()).to(torch.float64) / both.numel())
        for k, v in zip(("hd", "hd95", "assd", "nsd"), vals):
            out[k][p] = v
    return out
