"""Overlap and surface-distance measures between two masks, on top of the distance transform (vdr.morphology; the kernel is
csrc/edt.hip).  Plain torch in float64, per plane: masks are [P, H, W] or [H, W] on either device (a volume is compared slice by
slice), results are float64 / int64 tensors [P] on the masks' device.

The SURFACE of a mask is vdr.morphology.boundary: its set pixels with a clear 4-neighbour or on the plane's edge (medpy's
mask ^ binary_erosion(mask)).  The distance from a surface pixel of a to the surface of b is spacing * sqrt(float64(d2)), d2 the
exact squared distance to the nearest surface pixel of b (the transform of the complement of boundary(b)); it runs both ways.

Empty masks: two empty masks are a perfect match (dice = iou = nsd = 1, hd = hd95 = assd = 0).  ONE empty mask against a
non-empty one has no surface to measure to: hd = hd95 = assd = +inf and nsd = 0 (dice = iou = 0).

Parity with medpy, MONAI and DeepMind's surface-distance package is unpinned (none of them was at hand): the rules are restated
on scipy in the tests.

Volumes: surface(a, b, spacing=(sz, sy, sx)) takes the last three axes as ONE volume [Z, H, W] and gives one result per volume,
measured in 3-D and in spacing's unit: the surface is the 3-D boundary (the set voxels with a clear 6-neighbour or on a face), the
distances come from the 3-D transform (csrc/edt3d.hip) under the spacing rounded to the quantum 2^-10 (vdr.morphology.
quantize_spacing: exact for the rounded spacing), as sqrt(float64(d2)) * quantum.  Out of scope: spacing per volume of one call."""
from __future__ import annotations

import math

import torch

from . import components as cc
from . import morphology as mo


def _pair(a, b, what, volumes=False):
    ma, single = (cc.as_volumes if volumes else cc.as_planes)(a, what)
    mb, _ = (cc.as_volumes if volumes else cc.as_planes)(b, what)
    if ma.shape != mb.shape or ma.device != mb.device:
        raise ValueError(f"{what}: the two masks must have one shape and one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    return ma != 0, mb != 0


def overlap(a: torch.Tensor, b: torch.Tensor, volumes: bool = False) -> dict:
    """dice = 2 |a & b| / (|a| + |b|), iou = |a & b| / |a | b| (float64 [P]; 1 for two empty masks) and the three integer counts
    intersection, a and b (int64 [P]).  volumes=True: the masks are [Z, H, W] or [P, Z, H, W] and the counts are per volume.
    No synchronisation."""
    ma, mb = _pair(a, b, "overlap", volumes)
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


def _measures(ab: torch.Tensor, ba: torch.Tensor, near_ab, near_ba):
    """the four measures of one pair from the two one-way distance sets (float64) and the counts within the tolerance"""
    if ab.numel() == 0 and ba.numel() == 0:
        return (0.0, 0.0, 0.0, 1.0)
    if ab.numel() == 0 or ba.numel() == 0:
        return (math.inf, math.inf, math.inf, 0.0)
    both = torch.cat([ab, ba])
    # the count over the size as ONE IEEE division of two tensors (a division by a Python number may become a multiplication by its
    # reciprocal on the device): the same quotient on either device
    share = (near_ab + near_ba).to(torch.float64) / torch.full((), both.numel(), dtype=torch.float64, device=both.device)
    return (torch.maximum(ab.max(), ba.max()), percentile(both, 95.0), (ab.mean() + ba.mean()) / 2.0, share)


def _surface_volumes(a, b, spacing, tolerance) -> dict:
    """surface() for volumes: one result per volume, 3-D, in spacing's unit.  The tolerance is compared as an integer:
    d2 <= floor(tolerance^2 / quantum^2), which is sqrt(d2) * quantum <= tolerance without a rounding."""
    q, quantum = mo.quantize_spacing(spacing)
    t2 = mo.radius_squared("surface: tolerance", tolerance, quantum)
    ma, mb = _pair(a, b, "surface", volumes=True)
    mo.check_edt3("surface", q, 1, False, None, ma.shape[1:])
    P = ma.shape[0]
    sa, sb = mo.boundary(ma, spacing=spacing), mo.boundary(mb, spacing=spacing)
    to_a, to_b = mo._edt3(sa, q, 0, 0), mo._edt3(sb, q, 0, 0)         # the squared distance of every voxel to the surface of a / of b
    out = {k: torch.empty((P,), dtype=torch.float64, device=ma.device) for k in ("hd", "hd95", "assd", "nsd")}
    for p in range(P):
        d_ab, d_ba = to_b[p][sa[p]], to_a[p][sb[p]]
        vals = _measures(d_ab.to(torch.float64).sqrt() * float(quantum), d_ba.to(torch.float64).sqrt() * float(quantum), (d_ab <= t2).sum(), (d_ba <= t2).sum())
        for k, v in zip(("hd", "hd95", "assd", "nsd"), vals):
            out[k][p] = v
    return out


def surface(a: torch.Tensor, b: torch.Tensor, spacing=1.0, tolerance: float = 1.0) -> dict:
    """Surface distances between a and b, both ways, per plane (float64 [P]):
      hd    the larger of the two one-way maxima (the Hausdorff distance)
      hd95  the 95th percentile of the two one-way distance sets taken together, linear interpolation (medpy's hd95)
      assd  the mean of the two one-way means (the average symmetric surface distance)
      nsd   the share of the pixels of both surfaces that lie within `tolerance` of the other surface (surface Dice)
    spacing is the pixel size (one scalar), tolerance is in the same unit.  Two empty masks: 0, 0, 0, 1; one empty mask: inf, inf,
    inf, 0.  The surfaces have data-dependent sizes: this function synchronises once per plane.
    spacing=(sz, sy, sx): the masks are volumes [Z, H, W] or [P, Z, H, W] and the result is one per VOLUME (float64 [P]), from the
    3-D boundary into the 3-D transform; the empty-mask rules are the same."""
    if not isinstance(tolerance, (int, float)) or isinstance(tolerance, bool) or not tolerance >= 0:
        raise ValueError(f"surface: tolerance must be a number >= 0, got {tolerance!r}")
    if not isinstance(spacing, (int, float)):
        return _surface_volumes(a, b, spacing, tolerance)
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
