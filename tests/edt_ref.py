"""Reference side of the distance-transform tests: designed planes, scipy.ndimage.distance_transform_edt as the yardstick of d2,
brute force and a full separable evaluation in numpy for the tie rule of `nearest`, the disc, and the surface measures restated on
scipy.  Plain module, imported like components_ref.py; nothing here touches the library under test.

Everything is an integer: a plane is [H, W] uint8 (nonzero = set), `value` selects the measured pixels (1 the set, 0 the clear),
d2 is the squared distance to the nearest pixel that is not selected, NONE where there is none."""
import numpy as np

NONE = 2**31 - 1
# the strip lengths of the kernels (csrc/edt_map.h): 4 rows a row-pass workgroup, 16 rows and 64 columns a column-pass tile (and
# 64 segments a row), 256 threads a strided load / store loop
TS = (4, 16, 64, 256)
SIDES = sorted({s for T in TS for s in (1, 2, T - 1, T, T + 1, 2 * T + 1)})


def shapes():
    """every side as H and as W with several partners (a Latin arrangement, the non-square pairs included), a few squares, then
    the planes of the issue: two odd ones and the two that give the deepest search and the longest row"""
    n = len(SIDES)
    out = [(SIDES[a], SIDES[(a + 7) % n]) for a in range(n)] + [(SIDES[a], SIDES[(a + 13) % n]) for a in range(0, n, 2)]
    out += [(s, s) for s in (1, 2, 17, 64, 65)]
    return out + [(129, 257), (300, 517), (1, 4096), (4096, 1)]


def bernoulli(H, W, p, seed):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8)


def designed(H, W):
    """name -> plane (what is SET).  Every construction stays inside a 1 x 1 plane."""
    out = {}
    out["empty"] = np.zeros((H, W), np.uint8)
    out["full"] = np.ones((H, W), np.uint8)
    for name, (y0, x0) in (("clear_tl", (0, 0)), ("clear_tr", (0, W - 1)), ("clear_bl", (H - 1, 0)), ("clear_br", (H - 1, W - 1)),
                           ("clear_centre", (H // 2, W // 2))):
        m = np.ones((H, W), np.uint8)
        m[y0, x0] = 0
        out[name] = m
    m = np.ones((H, W), np.uint8)
    m[H // 2, :] = 0
    out["clear_row"] = m
    m = np.ones((H, W), np.uint8)
    m[:, W // 2] = 0
    out["clear_column"] = m
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = ((yy + xx) & 1).astype(np.uint8)
    # ties: the four corners clear (the middle row and column are equidistant from two of them), and two clear pixels of one row
    # an even gap apart plus two of one column (a band half-way between is equidistant)
    m = np.ones((H, W), np.uint8)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 0
    out["ties_corners"] = m
    m = np.ones((H, W), np.uint8)
    m[H // 3, W // 4] = m[H // 3, W // 4 + 2 * ((W - 1 - W // 4) // 4)] = 0
    m[H // 4, (2 * W) // 3] = m[H // 4 + 2 * ((H - 1 - H // 4) // 4), (2 * W) // 3] = 0
    out["ties_pairs"] = m
    # a clear pixel directly across every seam from a selected one: on the first column of every 64-column tile and of every row
    # segment, on the first row of every 4-row and 16-row strip
    m = np.ones((H, W), np.uint8)
    seg = (W + 63) // 64
    m[(yy % 7 == 0) & (xx % 64 == 0) & (xx > 0)] = 0
    m[(yy % 5 == 1) & (xx % seg == 0) & (xx > 0) & ((xx // seg) % 3 == 1)] = 0
    m[(yy % 4 == 0) & (yy > 0) & (xx % 11 == 3)] = 0
    out["seams"] = m
    # the row distance large and the column distance small, and the reverse
    m = np.ones((H, W), np.uint8)
    m[:, W - 1] = 0
    m[0, 0] = 0
    out["column_and_pixel"] = m
    m = np.ones((H, W), np.uint8)
    m[H - 1, :] = 0
    m[0, 0] = 0
    out["row_and_pixel"] = m
    return out


def planes(H, W):
    out = dict(designed(H, W))
    for p in (0.5, 0.99, 0.999):
        out[f"bernoulli{p}"] = bernoulli(H, W, p, int(p * 1000) + 3 * H + 7 * W)
    return out


def selected(mask, value):
    return (np.asarray(mask) != 0) == bool(value)


# ---- d2 -------------------------------------------------------------------------------------------------------------------------------
def scipy_d2(mask, value=1, outside=False):
    """rint(distance_transform_edt ^ 2) of the selected pixels as int32; `outside` by a plane padded with one non-selected pixel
    all round; NONE where nothing is non-selected (scipy leaves that case undefined)"""
    from scipy import ndimage
    sel = selected(mask, value)
    if outside:
        sel = np.pad(sel, 1)
    elif sel.all():
        return np.full(sel.shape, NONE, np.int32)
    d = ndimage.distance_transform_edt(sel)
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), d)          # scipy's float64 output is exactly sqrt(d2)
    return (d2[1:-1, 1:-1] if outside else d2).astype(np.int32)


def closed_form_outside_full(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx)) ** 2).astype(np.int32)


def brute(mask, value=1, outside=False):
    """(d2, nearest) by brute force over every non-selected pixel, the lowest index among the nearest (argmin takes the first)"""
    sel = selected(mask, value)
    H, W = sel.shape
    cy, cx = np.nonzero(~sel)                                            # in index order
    yy, xx = np.mgrid[0:H, 0:W]
    if cy.size:
        d = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
        k = d.argmin(axis=2)
        d2, nearest = np.take_along_axis(d, k[..., None], 2)[..., 0], cy[k] * W + cx[k]
    else:
        d2, nearest = np.full((H, W), NONE, np.int64), np.full((H, W), -1, np.int64)
    if outside:
        d2 = np.minimum(d2, closed_form_outside_full(H, W))
    return np.where(sel, d2, 0).astype(np.int32), np.where(sel, nearest, -1).astype(np.int32)


def row_offsets(sel):
    """per pixel the signed offset to the nearest non-selected pixel of its own row, the lower column on a tie; `none` where the
    row has no such pixel"""
    H, W = sel.shape
    xs = np.broadcast_to(np.arange(W), (H, W))
    far = 1 << 20
    last = np.maximum.accumulate(np.where(sel, -far, xs), axis=1)
    nxt = np.minimum.accumulate(np.where(sel, far, xs)[:, ::-1], axis=1)[:, ::-1]
    dl, dr = xs - last, nxt - xs
    return np.where(dl <= dr, -dl, dr), np.minimum(dl, dr) > 4096


def nearest_given_d2(mask, d2, value=1):
    """`nearest` under the tie rule, given the exact d2 (scipy's): the lowest row y' whose row distance attains d2, and in it the
    lower column.  Rows are tried at |y - y'| = 0, 1, .. floor(sqrt(max d2)); a plane with at most 8 non-selected pixels goes
    through brute force instead."""
    sel = selected(mask, value)
    H, W = sel.shape
    if (~sel).sum() <= 8:
        return brute(mask, value)[1]
    off, none = row_offsets(sel)
    g2 = np.where(none, np.int64(1) << 40, off.astype(np.int64) ** 2)
    d2 = d2.astype(np.int64)
    ynear = np.full((H, W), H, np.int64)
    yy = np.arange(H)[:, None]
    for k in range(int(np.sqrt(d2[sel].max(initial=0))) + 1):
        for s in (-k, k):
            rows = np.clip(yy + s, 0, H - 1)
            ok = ((yy + s >= 0) & (yy + s < H)) & (k * k + np.take_along_axis(g2, np.broadcast_to(rows, (H, W)), 0) == d2)
            ynear = np.where(ok, np.minimum(ynear, yy + s), ynear)
    assert (ynear[sel] < H).all()
    yn = np.clip(ynear, 0, H - 1)
    flat = yn * W + np.arange(W)[None, :] + np.take_along_axis(off, yn, 0)
    return np.where(sel, flat, -1).astype(np.int32)


def peak(d2):
    """(max d2, the lowest index that attains it), (0, -1) where d2 is 0 everywhere"""
    i = int(np.argmax(d2.reshape(-1)))                                  # the first maximum
    top = int(d2.reshape(-1)[i])
    return (top, i) if top > 0 else (0, -1)


# ---- morphology and measures on scipy -------------------------------------------------------------------------------------------------
def disc(r):
    """the Euclidean disc dy^2 + dx^2 <= floor(r^2) as a structuring element"""
    r2 = int(np.floor(float(r) * float(r)))
    k = int(np.floor(np.sqrt(r2)))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= r2


CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def surface_scipy(a, b, spacing=1.0, tolerance=1.0):
    """medpy's rules on scipy: the surface is mask ^ binary_erosion(mask, cross); the distances from one surface to the other come
    from distance_transform_edt of the other surface's complement with `sampling`; hd, hd95 (np.percentile, linear), assd, nsd"""
    from scipy import ndimage
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    sa, sb = a ^ ndimage.binary_erosion(a, CROSS), b ^ ndimage.binary_erosion(b, CROSS)
    if not sa.any() and not sb.any():
        return dict(hd=0.0, hd95=0.0, assd=0.0, nsd=1.0)
    if not sa.any() or not sb.any():
        return dict(hd=np.inf, hd95=np.inf, assd=np.inf, nsd=0.0)
    ab = ndimage.distance_transform_edt(~sb, sampling=spacing)[sa]
    ba = ndimage.distance_transform_edt(~sa, sampling=spacing)[sb]
    both = np.concatenate([ab, ba])
    return dict(hd=float(max(ab.max(), ba.max())), hd95=float(np.percentile(both, 95)), assd=float((ab.mean() + ba.mean()) / 2),
                nsd=float(((ab <= tolerance).sum() + (ba <= tolerance).sum()) / both.size))
