"""Euclidean distance transforms of mask planes and what rests on them (include/vdr.h "distance transform"; the kernels are
csrc/edt.hip and are reached through vdr.ops.distance_transform).

A plane is [H, W], nonzero = set, pixel index i = y * W + x.  d2 of a selected pixel is the squared distance to the nearest pixel
that is NOT selected -- an integer and a function of the mask alone, bit for bit rint(scipy.ndimage.distance_transform_edt ^ 2).

edt_torch states the op in plain torch (on the CPU unless told otherwise): the kernels are read against it bit for bit.  Every
other function here takes a mask on either device: on the HIP device it runs the kernel, on the CPU the statement, and the two
agree bit for bit.  Nothing here synchronises.

Volumes: with spacing=(sz, sy, sx) the last three axes of a mask are ONE volume [Z, H, W], voxel index i = (z H + y) W + x, and
distances are Euclidean under that voxel size (vdr_op_distance_transform_3d, csrc/edt3d.hip, reached through
vdr.ops.distance_transform_3d; edt3d_torch is its statement).  The op takes INTEGER spacing: quantize_spacing rounds a real
spacing to multiples of a quantum (2^-10 of its unit unless told otherwise), results are exact for the ROUNDED spacing, and a
radius r becomes r2 = floor(r^2 / quantum^2), evaluated exactly.  Without spacing every function is the 2-D one, plane by plane.

Out of scope: `nearest` in 3-D, spacing that differs per volume of one call, geodesic and chamfer distances, grey-scale
morphology."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from . import components as cc

NONE = 2**31 - 1        # VDR_EDT_NONE: a selected pixel with no candidate at all
_FAR = 1 << 20          # a column further away than any real one
_NO_ROW = 1 << 40       # the squared row distance of "none in this row" in the statement (int64: never overflows, never wins)
NONE3 = 2**63 - 1       # VDR_EDT3_NONE
MAX_Q = 65535           # VDR_EDT3_MAX_SPACING
MAX_D2 = 2**53          # (qz Z)^2 + (qy H)^2 + (qx W)^2 may not exceed it: exact in int64 and in float64
_INF3 = 1 << 61         # "no candidate yet" in the 3-D statement: three additions of less than 2^56 stay below 2^63


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


# ---- volumes: integer spacing, the checks, the torch statement --------------------------------------------------------------------
def quantize_spacing(spacing, quantum=2**-10):
    """A real voxel size (sz, sy, sx) -> ((qz, qy, qx), quantum) with q_a = round(s_a / quantum), evaluated exactly (ties to even);
    ValueError when a q_a leaves 1 .. 65535.  Everything computed with q is exact for the ROUNDED spacing q_a * quantum, which
    deviates from s_a by at most half a quantum: about half a micrometre for millimetre spacings at the default 2^-10."""
    try:
        sp = tuple(spacing)
    except TypeError:
        sp = ()
    ok = len(sp) == 3 and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0 for v in sp)
    if not ok:
        raise ValueError(f"quantize_spacing: spacing must be three finite numbers > 0 (sz, sy, sx), got {spacing!r}")
    if not (isinstance(quantum, (int, float)) and not isinstance(quantum, bool) and math.isfinite(quantum) and quantum > 0):
        raise ValueError(f"quantize_spacing: quantum must be a finite number > 0, got {quantum!r}")
    q = tuple(int(round(Fraction(v) / Fraction(quantum))) for v in sp)
    if not all(1 <= v <= MAX_Q for v in q):
        raise ValueError(f"quantize_spacing: spacing / quantum must round into 1 .. {MAX_Q}, got {q} for spacing {spacing!r} and quantum {quantum!r}")
    return q, quantum


def radius_squared(what: str, r, quantum) -> int:
    """r2 = floor(r^2 / quantum^2) of a real length r >= 0 in spacing's unit, evaluated exactly; or ValueError"""
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not (r >= 0) or math.isinf(r):
        raise ValueError(f"{what}: the radius must be a finite number >= 0, got {r!r}")
    r2 = math.floor(Fraction(r) ** 2 / Fraction(quantum) ** 2)
    if r2 > 2**62:
        raise ValueError(f"{what}: the radius is too large, got {r!r}")
    return int(r2)


def check_outside3(what: str, outside) -> int:
    """False / True / three bools (z, y, x) -> the op's bit mask: bit 2 = z, bit 1 = y, bit 0 = x"""
    if isinstance(outside, bool):
        return 7 if outside else 0
    try:
        o = tuple(outside)
    except TypeError:
        o = ()
    if len(o) != 3 or not all(isinstance(v, bool) for v in o):
        raise ValueError(f"{what}: outside must be a bool or three bools (z, y, x), got {outside!r}")
    return 4 * o[0] + 2 * o[1] + o[2]


def check_edt3(what: str, spacing, value, outside, threshold, shape=None):
    """((qz, qy, qx), value, outside bits, r2 or None) of a 3-D distance-transform call, or ValueError; with the volume's
    (Z, H, W) also the exactness bound (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53"""
    try:
        q = tuple(spacing)
    except TypeError:
        q = ()
    if len(q) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= MAX_Q for v in q):
        raise ValueError(f"{what}: spacing must be three integers (qz, qy, qx) in 1 .. {MAX_Q} (see quantize_spacing), got {spacing!r}")
    if isinstance(value, bool) or value not in (0, 1):
        raise ValueError(f"{what}: value must be 0 or 1, got {value!r}")
    bits = check_outside3(what, outside)
    if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, int) or not 0 <= threshold <= NONE3):
        raise ValueError(f"{what}: threshold must be an integer squared radius in 0 .. 2^63 - 1, got {threshold!r}")
    if shape is not None and sum((a * n) ** 2 for a, n in zip(q, shape)) > MAX_D2:
        raise ValueError(f"{what}: spacing {q} on a volume {tuple(shape)} exceeds (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53: distances would "
                         "not be exact; use a coarser quantum")
    return q, int(value), bits, threshold


def _min_plus(f: torch.Tensor, axis: int, q: int, outside: bool) -> torch.Tensor:
    """out[.., c, ..] = min over c' of f[.., c', ..] + (q (c - c'))^2 along `axis`, all of it, no early stop; with `outside` also
    over (q (c + 1))^2 and (q (n - c))^2"""
    f = f.movedim(axis, -1).contiguous()
    n = f.shape[-1]
    c = torch.arange(n, dtype=torch.int64, device=f.device)
    w = (q * (c[:, None] - c[None, :])) ** 2
    flat = f.reshape(-1, n)
    out = torch.empty_like(flat)
    step = max(1, (1 << 22) // (n * n))                                    # at most 2^22 candidates at a time
    for i0 in range(0, flat.shape[0], step):
        out[i0:i0 + step] = (flat[i0:i0 + step, None, :] + w[None]).min(dim=2).values
    if outside:
        out = torch.minimum(out, ((q * torch.minimum(c + 1, n - c)) ** 2)[None])
    return out.clamp_max(_INF3).reshape(f.shape).movedim(-1, axis)


def edt3d_torch(vol: torch.Tensor, spacing=(1, 1, 1), value: int = 1, outside=False, return_peak: bool = False, device="cpu"):
    """vdr_op_distance_transform_3d in torch, on the CPU unless told otherwise: the separable form in int64, one axis after the
    other, every candidate of a line (dense: it is for small volumes).  vol [Z, H, W] or [P, Z, H, W] -> d2 int64 like vol, then
    peak int64 [P, 2] where asked for, as vdr.ops.distance_transform_3d returns them."""
    v, single = cc.as_volumes(vol.detach().to(device) if isinstance(vol, torch.Tensor) else vol, "edt3d_torch")
    q, value, bits, _ = check_edt3("edt3d_torch", spacing, value, outside, None, v.shape[1:])
    sel = (v != 0) == bool(value)
    f = torch.where(sel, torch.full((), _INF3, dtype=torch.int64, device=v.device), torch.zeros((), dtype=torch.int64, device=v.device))
    for axis, qa, bit in ((3, q[2], 1), (2, q[1], 2), (1, q[0], 4)):
        f = _min_plus(f, axis, qa, bool(bits & bit))
    d2 = torch.where(sel, torch.where(f >= _INF3, torch.full_like(f, NONE3), f), torch.zeros_like(f))
    out = [d2[0] if single else d2]
    if return_peak:
        out.append(peak3_torch(d2))
    return out[0] if len(out) == 1 else tuple(out)


def peak3_torch(d2: torch.Tensor) -> torch.Tensor:
    """d2 int64 [P, Z, H, W] -> int64 [P, 2]: the largest d2 and the lowest voxel index that attains it; (0, -1) where d2 is 0
    everywhere.  Pure torch on d2's device, no synchronisation."""
    P = d2.shape[0]
    flat = d2.reshape(P, -1)
    n = flat.shape[1]
    top = flat.max(dim=1).values
    idx = torch.where(flat == top[:, None], torch.arange(n, device=d2.device)[None], torch.full((), n, dtype=torch.int64, device=d2.device)).min(dim=1).values
    return torch.stack([top, torch.where(top > 0, idx, torch.full_like(idx, -1))], dim=1)


def _edt3(vol, q, value, outside, threshold=None, peak=False):
    """d2 (or the thresholded volume), or the peak alone, of a volume mask on either device: the kernel on the HIP device, the
    statement on the CPU.  outside: the op's bits"""
    o3 = (bool(outside & 4), bool(outside & 2), bool(outside & 1))
    if vol.is_cuda:
        from . import ops
        if peak:
            return ops.distance_transform_3d(vol, q, value, o3, return_peak=True, return_d2=False)
        return ops.distance_transform_3d(vol, q, value, o3, threshold=threshold)
    if peak:
        return edt3d_torch(vol, q, value, o3, return_peak=True)[1]
    d2 = edt3d_torch(vol, q, value, o3)
    return d2 if threshold is None else (d2 <= threshold).to(torch.uint8)


def _volume(what: str, mask, spacing, r=None):
    """the checks of a morphology call with spacing: ((qz, qy, qx), quantum, r2 or None), the operand and the exactness bound"""
    q, quantum = quantize_spacing(spacing)
    r2 = None if r is None else radius_squared(what, r, quantum)
    v, _ = cc.as_volumes(mask, what)
    check_edt3(what, q, 1, False, None, v.shape[1:])
    return q, quantum, r2


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
def dilate(mask: torch.Tensor, r: float, spacing=None) -> torch.Tensor:
    """Euclidean dilation by the disc of radius r (a real number >= 0, compared as floor(r^2)): the pixels within r of a set
    pixel -- ONE transform of the clear pixels, thresholded; scipy.ndimage.binary_dilation with the disc as structure.  The
    result has the mask's type (bool or uint8 0 / 1); r = 0 returns the mask.
    spacing=(sz, sy, sx): the last three axes are one volume, r is a length in spacing's unit and the structure is the ellipsoid
    (qz dz)^2 + (qy dy)^2 + (qx dx)^2 <= r2 of quantize_spacing and radius_squared -- still ONE thresholded transform."""
    if spacing is not None:
        q, _, r2 = _volume("dilate", mask, spacing, r)
        return mask if r2 == 0 else _like(_edt3(mask, q, 0, 0, r2), mask)
    cc.as_planes(mask, "dilate")
    r2 = check_radius("dilate", r)
    return mask if r2 == 0 else _like(_edt(mask, 0, False, r2), mask)


def erode(mask: torch.Tensor, r: float, outside=True, spacing=None) -> torch.Tensor:
    """Euclidean erosion by the disc of radius r: the set pixels further than r from every clear pixel -- ONE transform of the set
    pixels.  outside=True (the default; scipy.ndimage.binary_erosion's border_value=0): the plane's outside erodes too.
    spacing=(sz, sy, sx): a volume and the ellipsoid, as in dilate; outside may then be three bools (z, y, x)."""
    if spacing is not None:
        q, _, r2 = _volume("erode", mask, spacing, r)
        bits = check_outside3("erode", outside)
        return mask if r2 == 0 else _like(_edt3(mask, q, 1, bits, r2) == 0, mask)
    cc.as_planes(mask, "erode")
    r2 = check_radius("erode", r)
    return mask if r2 == 0 else _like(_edt(mask, 1, bool(outside), r2) == 0, mask)


def opening(mask: torch.Tensor, r: float, outside=True, spacing=None) -> torch.Tensor:
    """dilate(erode(mask, r, outside), r): parts narrower than the disc (with spacing: the ellipsoid) go"""
    return dilate(erode(mask, r, outside, spacing), r, spacing)


def closing(mask: torch.Tensor, r: float, outside=False, spacing=None) -> torch.Tensor:
    """erode(dilate(mask, r), r, outside): gaps narrower than the disc close.  outside=False (the default) keeps what touches the
    plane's edge; outside=True is scipy.ndimage.binary_closing, whose erosion also eats in from the edge."""
    return erode(dilate(mask, r, spacing), r, outside, spacing)


def ring(mask: torch.Tensor, inner: float, outer: float, spacing=None) -> torch.Tensor:
    """dilate(mask, outer) without dilate(mask, inner), 0 <= inner < outer: the peritumoral ring (inner = 0: the dilation without
    the mask).  One transform of the clear pixels.  spacing=(sz, sy, sx): the shell between two ellipsoids of a volume."""
    if spacing is not None:
        q, quantum, i2 = _volume("ring", mask, spacing, inner)
        o2 = radius_squared("ring", outer, quantum)
        if not i2 < o2:
            raise ValueError(f"ring: floor(inner^2 / quantum^2) must be below floor(outer^2 / quantum^2), got {inner!r} and {outer!r}")
        d2 = _edt3(mask, q, 0, 0)
        return _like((d2 > i2) & (d2 <= o2), mask)
    cc.as_planes(mask, "ring")
    i2, o2 = check_radius("ring", inner), check_radius("ring", outer)
    if not i2 < o2:
        raise ValueError(f"ring: floor(inner^2) must be below floor(outer^2), got {inner!r} and {outer!r}")
    d2 = _edt(mask, 0, False)
    return _like((d2 > i2) & (d2 <= o2), mask)


def boundary(mask: torch.Tensor, spacing=None) -> torch.Tensor:
    """The set pixels with a clear 4-neighbour or on the plane's edge: mask & (d2(outside) == 1), which is
    mask ^ binary_erosion(mask, cross) -- how medpy takes a surface.  With a spacing (any: only "the last three axes are one
    volume" is read from it) the set voxels with a clear 6-neighbour or on one of the volume's faces: d2 == 1 at UNIT spacing with
    all `outside` bits set, mask ^ binary_erosion(mask, the 6-neighbour cross)."""
    if spacing is not None:
        _volume("boundary", mask, spacing)
        return _like((mask != 0) & (_edt3(mask, (1, 1, 1), 1, 7, 1) != 0), mask)
    cc.as_planes(mask, "boundary")
    return _like((mask != 0) & (_edt(mask, 1, True, 1) != 0), mask)


def signed_distance(mask: torch.Tensor, spacing=None) -> torch.Tensor:
    """fp32 like mask: +sqrt(d2) on the set pixels, -sqrt(d2 of the clear pixels) on the clear ones (the square root in double,
    rounded once to fp32); +inf / -inf on a plane that is all set / all clear.  spacing=(sz, sy, sx): a volume, the distance
    sqrt(d2) * quantum in spacing's unit (double, then one rounding to fp32)."""
    if spacing is not None:
        q, quantum, _ = _volume("signed_distance", mask, spacing)
        d2 = torch.where(mask != 0, _edt3(mask, q, 1, 0), _edt3(mask, q, 0, 0))
        d = torch.where(d2 == NONE3, torch.full((), float("inf"), dtype=torch.float64, device=mask.device), d2.to(torch.float64).sqrt() * float(quantum))
        return torch.where(mask != 0, d, -d).to(torch.float32)
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


def inner_voxel(mask: torch.Tensor, spacing, outside=True):
    """The most interior voxel of every volume: the peak of the 3-D distance transform of the set voxels under spacing (the lowest
    voxel index on a tie) -> (zyx int64 [P, 3], labels int32 [P]).  The label is 1, or -1 with voxel (0, 0, 0) for a volume with
    nothing set.  z is the slice to start a propagation sweep from, (x, y) the click in it.  outside=True (or three bools
    (z, y, x)): the volume's faces count as clear, so the voxel keeps away from them too.  No synchronisation."""
    q, _, _ = _volume("inner_voxel", mask, spacing)
    bits = check_outside3("inner_voxel", outside)
    v, _ = cc.as_volumes(mask, "inner_voxel")
    H, W = int(v.shape[2]), int(v.shape[3])
    idx = _edt3(mask, q, 1, bits, peak=True)[:, 1]
    has = idx >= 0
    i = idx.clamp_min(0)
    zyx = torch.stack([i // (H * W), (i // W) % H, i % W], dim=1) * has[:, None].to(torch.int64)
    return zyx, torch.where(has, torch.ones_like(idx), -torch.ones_like(idx)).to(torch.int32)
