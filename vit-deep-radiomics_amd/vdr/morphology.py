"""Euclidean distance transforms of mask planes and what rests on them (include/vdr.h "distance transform"; the kernels are
csrc/edt.hip and are reached through vdr.ops.distance_transform).

A plane is [H, W], nonzero = set, pixel index i = y * W + x.  d2 of a selected pixel is the squared distance to the nearest pixel
that is NOT selected -- an integer and a function of the mask alone, bit for bit rint(scipy.ndimage.distance_transform_edt ^ 2).

edt_torch states the op in plain torch (on the CPU unless told otherwise): the kernels are read against it bit for bit.  Every
other function here takes a mask on either device: on the HIP device it runs the kernel, on the CPU the statement, and the two
agree bit for bit.  Nothing here synchronises.

Out of scope: 3-D transforms and anisotropic spacing (a volume is treated slice by slice), geodesic and chamfer distances,
grey-scale morphology."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import components as cc

NONE = 2**31 - 1        # VDR_EDT_NONE: a selected pixel with no candidate at all
_FAR = 1 << 20          # a column further away than any real one
_NO_ROW = 1 << 40       # the squared row distance of "none in this row" in the statement (int64: never overflows, never wins)


def check_edt(what: str, value, outside, return_nearest, threshold):
    """(value, outside, r2 or None) of a distance-transform call, or ValueError"""
    if isinstance(value, bool) or value not in (0, 1):
        raise ValueError(f"{what}: value must be 0 or 1, got {value!r}")
    if not isinstance(outside, (bool, int)) or outside not in (0, 1):
        raise ValueError(f"{what}: outside must be a bool, got {outside!r}")
    if return_nearest and outside:
        raise ValueError(f"{what}: nearest is not defined with outside=True (the nearest point may lie beyond the plane)")
    if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, int) or not 0 <= threshold <= NONE):
        raise ValueError(f"{what}: threshold must be an integer squared radius in 0 .. 2^31 - 1, got {threshold!r}")
    return int(value), int(bool(outside)), threshold


def check_radius(what: str, r) -> int:
    """floor(r^2) of a real radius r >= 0 (r * r in double, then the floor), or ValueError"""
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not (r >= 0) or math.isinf(r):
        raise ValueError(f"{what}: the radius must be a finite number >= 0, got {r!r}")
    r2 = math.floor(float(r) * float(r))
    if r2 > NONE - 1:
        raise ValueError(f"{what}: the radius is too large, got {r!r}")
    return int(r2)


# ---- the torch statement --------------------------------------------------------------------------------------------------------
def edt_torch(mask: torch.Tensor, value: int = 1, outside: bool = False, return_nearest: bool = False, return_peak: bool = False, device="cpu"):
    """vdr_op_distance_transform in torch, on the CPU unless told otherwise, in the separable form: per pixel the signed offset
    to the nearest non-selected pixel of its own row (cummax / cummin; the lower column on a tie), then per pixel the minimum
    over the rows y' of (y - y')^2 + offset(y', x)^2 (the lowest y' on a tie).  mask [P, H, W] or [H, W] -> d2 int32, then
    nearest int32 and peak int32 [P, 2] where asked for, as vdr.ops.distance_transform returns them."""
    m, single = cc.as_planes(mask.detach().to(device), "edt_torch")
    value, outside, _ = check_edt("edt_torch", value, outside, return_nearest, None)
    P, H, W = m.shape
    dev = m.device
    sel = (m != 0) == bool(value)
    xs = torch.arange(W, dtype=torch.int64, device=dev).expand(P, H, W)
    far = torch.full((), _FAR, dtype=torch.int64, device=dev)
    last = torch.cummax(torch.where(sel, -far, xs), dim=2).values
    nxt = torch.cummin(torch.where(sel, far, xs).flip(2), dim=2).values.flip(2)
    if outside:
        last, nxt = last.clamp_min(-1), nxt.clamp_max(W)
    dl, dr = xs - last, nxt - xs
    off = torch.where(dl <= dr, -dl, dr)                                   # the lower column on a tie
    g2 = torch.where(torch.minimum(dl, dr) > 4096, torch.full((), _NO_ROW, dtype=torch.int64, device=dev), off * off)
    ys = torch.arange(H, dtype=torch.int64, device=dev)
    d2 = torch.empty((P, H, W), dtype=torch.int64, device=dev)
    yn = torch.empty((P, H, W), dtype=torch.int64, device=dev)
    step = max(1, (1 << 22) // max(1, P * H * W))                           # rows of y per chunk: at most 2^22 candidates at a time
    for y0 in range(0, H, step):
        y1 = min(H, y0 + step)
        dy = ys[y0:y1, None] - ys[None, :]                                  # [c, H]
        key = ((dy * dy)[None, :, :, None] + g2[:, None, :, :]) * 4096 + ys[None, None, :, None]   # cost first, then the lower row
        best = key.min(dim=2).values
        d2[:, y0:y1], yn[:, y0:y1] = best // 4096, best % 4096
    none = d2 >= _NO_ROW
    if outside:
        by = torch.minimum(ys + 1, H - ys)
        d2 = torch.minimum(d2, (by * by)[None, :, None].expand(P, H, W))
    flat = (yn * W + xs + torch.gather(off, 1, yn)).to(torch.int64)
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    d2 = torch.where(sel, torch.where(none & (d2 >= _NO_ROW), torch.full((), NONE, dtype=torch.int64, device=dev), d2), zero)
    out = [d2.to(torch.int32)[0] if single else d2.to(torch.int32)]
    if return_nearest:
        nearest = torch.where(sel & ~none, flat, zero - 1).to(torch.int32)
        out.append(nearest[0] if single else nearest)
    if return_peak:
        out.append(peak_torch(d2.to(torch.int32)))
    return out[0] if len(out) == 1 else tuple(out)


def peak_torch(d2: torch.Tensor) -> torch.Tensor:
    """d2 int32 [P, H, W] -> int32 [P, 2]: the largest d2 and the lowest pixel index that attains it; (0, -1) where d2 is 0
    everywhere.  Pure torch on d2's device, no synchronisation."""
    P = d2.shape[0]
    flat = d2.reshape(P, -1).to(torch.int64)
    n = flat.shape[1]
    key = flat * n + (n - 1 - torch.arange(n, device=d2.device))            # the larger d2 first, then the lower index
    best = key.argmax(dim=1)
    top = flat.gather(1, best[:, None])[:, 0]
    return torch.stack([top, torch.where(top > 0, best, torch.full_like(best, -1))], dim=1).to(torch.int32)


def _edt(mask, value, outside, threshold=None, peak=False):
    """d2 (or the thresholded plane), or the peak alone, of a mask on either device: the kernel on the HIP device, the statement
    on the CPU"""
    if mask.is_cuda:
        from . import ops
        if peak:
            return ops.distance_transform(mask, value, outside, return_peak=True, return_d2=False)   # the peak alone: no plane is written
        return ops.distance_transform(mask, value, outside, threshold=threshold)
    if peak:
        return edt_torch(mask, value, outside, return_peak=True)[1]
    d2 = edt_torch(mask, value, outside)
    return d2 if threshold is None else (d2 <= threshold).to(torch.uint8)


def _like(out: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return out.to(torch.bool) if mask.dtype == torch.bool else out.to(torch.uint8)


# ---- morphology with the Euclidean disc dy^2 + dx^2 <= r^2 ----------------------------------------------------------------------
def dilate(mask: torch.Tensor, r: float) -> torch.Tensor:
    """Euclidean dilation by the disc of radius r (a real number >= 0, compared as floor(r^2)): the pixels within r of a set
    pixel -- ONE transform of the clear pixels, thresholded; scipy.ndimage.binary_dilation with the disc as structure.  The
    result has the mask's type (bool or uint8 0 / 1); r = 0 returns the mask."""
    cc.as_planes(mask, "dilate")
    r2 = check_radius("dilate", r)
    return mask if r2 == 0 else _like(_edt(mask, 0, False, r2), mask)


def erode(mask: torch.Tensor, r: float, outside: bool = True) -> torch.Tensor:
    """Euclidean erosion by the disc of radius r: the set pixels further than r from every clear pixel -- ONE transform of the set
    pixels.  outside=True (the default; scipy.ndimage.binary_erosion's border_value=0): the plane's outside erodes too."""
    cc.as_planes(mask, "erode")
    r2 = check_radius("erode", r)
    return mask if r2 == 0 else _like(_edt(mask, 1, bool(outside), r2) == 0, mask)


def opening(mask: torch.Tensor, r: float, outside: bool = True) -> torch.Tensor:
    """dilate(erode(mask, r, outside), r): parts narrower than the disc go"""
    return dilate(erode(mask, r, outside), r)


def closing(mask: torch.Tensor, r: float, outside: bool = False) -> torch.Tensor:
    """erode(dilate(mask, r), r, outside): gaps narrower than the disc close.  outside=False (the default) keeps what touches the
    plane's edge; outside=True is scipy.ndimage.binary_closing, whose erosion also eats in from the edge."""
    return erode(dilate(mask, r), r, outside)


def ring(mask: torch.Tensor, inner: float, outer: float) -> torch.Tensor:
    """dilate(mask, outer) without dilate(mask, inner), 0 <= inner < outer: the peritumoral ring (inner = 0: the dilation without
    the mask).  One transform of the clear pixels."""
    cc.as_planes(mask, "ring")
    i2, o2 = check_radius("ring", inner), check_radius("ring", outer)
    if not i2 < o2:
        raise ValueError(f"ring: floor(inner^2) must be below floor(outer^2), got {inner!r} and {outer!r}")
    d2 = _edt(mask, 0, False)
    return _like((d2 > i2) & (d2 <= o2), mask)


def boundary(mask: torch.Tensor) -> torch.Tensor:
    """The set pixels with a clear 4-neighbour or on the plane's edge: mask & (d2(outside) == 1), which is
    mask ^ binary_erosion(mask, cross) -- how medpy takes a surface."""
    cc.as_planes(mask, "boundary")
    return _like((mask != 0) & (_edt(mask, 1, True, 1) != 0), mask)


def signed_distance(mask: torch.Tensor) -> torch.Tensor:
    """fp32 like mask: +sqrt(d2) on the set pixels, -sqrt(d2 of the clear pixels) on the clear ones (the square root in double,
    rounded once to fp32); +inf / -inf on a plane that is all set / all clear"""
    cc.as_planes(mask, "signed_distance")
    inside, outside_ = _edt(mask, 1, False), _edt(mask, 0, False)
    d2 = torch.where(mask != 0, inside, outside_)
    d = torch.where(d2 == NONE, torch.full((), float("inf"), dtype=torch.float64, device=mask.device), d2.to(torch.float64).sqrt())
    return torch.where(mask != 0, d, -d).to(torch.float32)


def points_of_peak(peak: torch.Tensor, H: int, W: int, img=None):
    """peak int32 [P, 2] of H x W planes -> (points fp32 [P, 2] (x, y), labels int32 [P]).  The point of peak index i on a plane
    that stands for an img-pixel input is ((x + 0.5) * s - 0.5, (y + 0.5) * s - 0.5) with s = img / W (img / H for y) in fp32,
    every operation rounded once (SAM's prompt encoder adds the 0.5 back); img None: the plane's own pixels.  The label is 1,
    or -1 ("not a point", point (0, 0)) where the peak has no index."""
    ih, iw = (H, W) if img is None else ((int(img), int(img)) if isinstance(img, int) else (int(img[0]), int(img[1])))
    idx = peak[:, 1].to(torch.int64)
    has = idx >= 0
    i = idx.clamp_min(0)
    sx, sy = float(np.float32(iw) / np.float32(W)), float(np.float32(ih) / np.float32(H))   # fp32 quotients, exact as Python floats
    x = ((i % W).to(torch.float32) + 0.5) * sx - 0.5
    y = ((i // W).to(torch.float32) + 0.5) * sy - 0.5
    pts = torch.stack([x, y], dim=1) * has[:, None].to(torch.float32)
    lab = torch.where(has, torch.ones_like(idx), -torch.ones_like(idx)).to(torch.int32)
    return pts, lab


def inner_point(mask: torch.Tensor, img=None, outside: bool = True):
    """The most interior pixel of every plane as a point prompt: the peak of the distance transform of the set pixels (the lowest
    index on a tie) -> (points fp32 [P, 2] (x, y), labels int32 [P]), see points_of_peak.  outside=True: the plane's edge counts
    as clear, so the point keeps away from it too.  No synchronisation."""
    m, _ = cc.as_planes(mask, "inner_point")
    return points_of_peak(_edt(mask, 1, bool(outside), peak=True), int(m.shape[1]), int(m.shape[2]), img)
