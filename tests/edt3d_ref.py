"""Reference side of the 3-D distance-transform tests: designed volumes, scipy.ndimage.distance_transform_edt with `sampling=` as
the yardstick of d2, integer brute force, the ellipsoid, the 6-neighbour cross, and the surface measures restated on scipy.  Plain
module, imported like edt_ref.py; nothing here touches the library under test.

A volume is [Z, H, W] uint8 (nonzero = set), voxel index (z H + y) W + x, `value` selects the measured voxels (1 the set, 0 the
clear), spacing q = (qz, qy, qx) integers, d2 = min (qz dz)^2 + (qy dy)^2 + (qx dx)^2 to a voxel that is not selected, NONE
where there is none.  `outside` is the op's bit mask: bit 2 = z, bit 1 = y, bit 0 = x."""
from fractions import Fraction

import numpy as np

NONE = 2**63 - 1
SPACINGS = [(1, 1, 1), (3, 1, 1), (1, 2, 5), (2560, 717, 717), (65535, 1, 300)]


def exact(shape, q):
    """the op's bound: (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53"""
    return sum((int(a) * int(n)) ** 2 for a, n in zip(q, shape)) <= 2**53


def bits3(outside):
    return (bool(outside & 4), bool(outside & 2), bool(outside & 1))


def selected(vol, value):
    return (np.asarray(vol) != 0) == bool(value)


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def designed(Z, H, W):
    """name -> volume (what is SET).  Every construction stays inside a 1 x 1 x 1 volume."""
    out = {}
    out["none_set"] = np.zeros((Z, H, W), np.uint8)
    out["all_set"] = np.ones((Z, H, W), np.uint8)
    for c in range(8):                                                    # one clear voxel at each corner ...
        m = np.ones((Z, H, W), np.uint8)
        m[(Z - 1) * (c >> 2 & 1), (H - 1) * (c >> 1 & 1), (W - 1) * (c & 1)] = 0
        out[f"clear_corner{c}"] = m
    m = np.ones((Z, H, W), np.uint8)                                      # ... and at the centre
    m[Z // 2, H // 2, W // 2] = 0
    out["clear_centre"] = m
    m = np.ones((Z, H, W), np.uint8)                                      # a clear slab on a z seam: the slice in the middle
    m[Z // 2] = 0
    out["clear_slab"] = m
    zz, yy, xx = np.mgrid[0:Z, 0:H, 0:W]
    out["checkerboard"] = ((zz + yy + xx) & 1).astype(np.uint8)
    return out


def volumes(Z, H, W):
    out = dict(designed(Z, H, W))
    for p in (0.5, 0.9, 0.99):
        out[f"bernoulli{p}"] = bernoulli((Z, H, W), p, int(p * 100) + 3 * Z + 5 * H + 7 * W)
    return out


# ---- d2 -------------------------------------------------------------------------------------------------------------------------------
def scipy_d2(vol, q=(1, 1, 1), value=1, outside=0):
    """rint(distance_transform_edt(selected, sampling=q) ^ 2) as int64; an `outside` axis by padding it with one non-selected
    voxel on either side; NONE where nothing is non-selected (scipy leaves that case undefined).  Asserts that scipy's float64
    output is exactly sqrt(d2): the bound of `exact` is what makes it so."""
    from scipy import ndimage
    sel = selected(vol, value)
    assert exact(sel.shape, q)
    o3 = bits3(outside)
    if outside:
        sel = np.pad(sel, [(1, 1) if b else (0, 0) for b in o3])
    if sel.all():
        return np.full(sel.shape, NONE, np.int64)
    d = ndimage.distance_transform_edt(sel, sampling=[float(v) for v in q])
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), d)
    return d2[tuple(slice(1, -1) if b else slice(None) for b in o3)]


def brute(vol, q=(1, 1, 1), value=1, outside=0):
    """d2 by integer brute force (Python ints: no overflow anywhere) over every non-selected voxel and the faces of `outside`"""
    sel = selected(vol, value)
    Z, H, W = sel.shape
    cand = np.argwhere(~sel).astype(object)
    qq = np.array([int(v) for v in q], dtype=object)
    out = np.zeros((Z, H, W), np.int64)
    for z, y, x in np.argwhere(sel):
        best = NONE
        if len(cand):
            best = min(best, int((((cand - np.array([z, y, x], dtype=object)) * qq) ** 2).sum(axis=1).min()))
        for bit, c, n, a in ((4, z, Z, q[0]), (2, y, H, q[1]), (1, x, W, q[2])):
            if outside & bit:
                best = min(best, (int(a) * (int(c) + 1)) ** 2, (int(a) * (n - int(c))) ** 2)
        out[z, y, x] = best
    return out


def peak(d2):
    """(max d2, the lowest voxel index that attains it), (0, -1) where d2 is 0 everywhere"""
    i = int(np.argmax(d2.reshape(-1)))                                  # the first maximum
    top = int(d2.reshape(-1)[i])
    return (top, i) if top > 0 else (0, -1)


# ---- morphology and measures on scipy -------------------------------------------------------------------------------------------------
def quantize(spacing, quantum=Fraction(1, 1024)):
    return tuple(int(round(Fraction(s) / Fraction(quantum))) for s in spacing)


def radius2(r, quantum=Fraction(1, 1024)):
    return int(Fraction(r) ** 2 / Fraction(quantum) ** 2 // 1)


def ellipsoid(q, r2, shape):
    """{(dz, dy, dx): (qz dz)^2 + (qy dy)^2 + (qx dx)^2 <= r2} as a structuring element, cut to the offsets that exist inside a
    volume of `shape` (and one beyond, for the border)"""
    import math
    k = [min(math.isqrt(int(r2)) // int(a), int(n)) for a, n in zip(q, shape)]
    zz, yy, xx = np.mgrid[-k[0]:k[0] + 1, -k[1]:k[1] + 1, -k[2]:k[2] + 1]
    return (q[0] * zz) ** 2 + (q[1] * yy) ** 2 + (q[2] * xx) ** 2 <= r2


CROSS6 = np.zeros((3, 3, 3), bool)
CROSS6[1, 1, :] = CROSS6[1, :, 1] = CROSS6[:, 1, 1] = True


def surface_scipy(a, b, spacing, tolerance=1.0, quantum=Fraction(1, 1024)):
    """the 2-D restatement one dimension up: the surface is mask ^ binary_erosion(mask, 6-cross); the distances from one surface to
    the other come from distance_transform_edt of the other surface's complement with sampling = the quantized spacing, times the
    quantum; hd, hd95 (np.percentile, linear), assd; nsd counts rint(d^2) <= floor(tolerance^2 / quantum^2)"""
    from scipy import ndimage
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    q = quantize(spacing, quantum)
    sa, sb = a ^ ndimage.binary_erosion(a, CROSS6), b ^ ndimage.binary_erosion(b, CROSS6)
    if not sa.any() and not sb.any():
        return dict(hd=0.0, hd95=0.0, assd=0.0, nsd=1.0)
    if not sa.any() or not sb.any():
        return dict(hd=np.inf, hd95=np.inf, assd=np.inf, nsd=0.0)
    ab = ndimage.distance_transform_edt(~sb, sampling=[float(v) for v in q])[sa]
    ba = ndimage.distance_transform_edt(~sa, sampling=[float(v) for v in q])[sb]
    t2 = radius2(tolerance, quantum)
    near = int((np.rint(ab * ab).astype(np.int64) <= t2).sum() + (np.rint(ba * ba).astype(np.int64) <= t2).sum())
    ab, ba = ab * float(quantum), ba * float(quantum)
    both = np.concatenate([ab, ba])
    return dict(hd=float(max(ab.max(), ba.max())), hd95=float(np.percentile(both, 95)), assd=float((ab.mean() + ba.mean()) / 2), nsd=near / both.size)
