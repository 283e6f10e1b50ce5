"""Reference statements for the connected-component tests (helper, not collected): two independent labellings in numpy -- a
two-pass union-find and a breadth-first search -- the clean rules of vdr_op_mask_clean restated on top of a root plane, and the
designed planes.  A plane is [H, W], nonzero = set, pixel index i = y * W + x; root = the lowest index of the component, -1
where the pixel is not selected; area = the component's pixel count at its root."""
from collections import deque

import numpy as np

T = 64   # the kernels' tile side (csrc/components_map.h CC_T): the designed planes put their features on its seams


# ---- two labellings ------------------------------------------------------------------------------------------------------------------
def roots_union_find(mask, connectivity=8, value=1):
    """Two-pass union-find: pass 1 unions every selected pixel with its selected W, N (and NW, NE) neighbours, the smaller root
    winning; pass 2 resolves every pixel.  -> (root int32 [H, W], area int32 [H, W], count)"""
    sel = (np.asarray(mask) != 0) == bool(value)
    H, W = sel.shape
    parent = np.arange(H * W, dtype=np.int64)

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r
    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    ys, xs = np.nonzero(sel)
    for y, x in zip(ys.tolist(), xs.tolist()):
        for dy, dx in back:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and sel[yy, xx]:
                a, b = find(y * W + x), find(yy * W + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.full(H * W, -1, dtype=np.int32)
    for y, x in zip(ys.tolist(), xs.tolist()):
        root[y * W + x] = find(y * W + x)
    area = np.bincount(root[root >= 0], minlength=H * W).astype(np.int32)
    return root.reshape(H, W), area.reshape(H, W), int((area > 0).sum())


def roots_bfs(mask, connectivity=8, value=1):
    """Breadth-first search from every unvisited selected pixel in index order: the start is the component's lowest index"""
    sel = (np.asarray(mask) != 0) == bool(value)
    H, W = sel.shape
    root = np.full((H, W), -1, dtype=np.int32)
    area = np.zeros((H, W), dtype=np.int32)
    nb = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    count = 0
    for y0, x0 in zip(*(a.tolist() for a in np.nonzero(sel))):
        if root[y0, x0] >= 0:
            continue
        s, n = y0 * W + x0, 0
        root[y0, x0] = s
        q = deque([(y0, x0)])
        while q:
            y, x = q.popleft()
            n += 1
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and sel[yy, xx] and root[yy, xx] < 0:
                    root[yy, xx] = s
                    q.append((yy, xx))
        area[y0, x0] = n
        count += 1
    return root, area, count


def roots_from_labels(lab):
    """A label plane (0 = not selected, equal positive labels = one component; scipy.ndimage.label's output) -> (root, area,
    count): the first index of every label"""
    lab = np.asarray(lab)
    H, W = lab.shape
    flat = lab.reshape(-1)
    n = int(flat.max()) if flat.size else 0
    first = np.full(n + 1, -1, dtype=np.int64)
    idx = np.nonzero(flat)[0]
    first[flat[idx][::-1]] = idx[::-1]            # the last write is the lowest index
    root = np.where(flat > 0, first[flat], -1).astype(np.int32)
    area = np.zeros(H * W, dtype=np.int32)
    cnt = np.bincount(flat, minlength=n + 1)
    area[first[1:]] = cnt[1:]
    return root.reshape(H, W), area.reshape(H, W), n


def scipy_roots(mask, connectivity=8, value=1):
    from scipy import ndimage
    sel = (np.asarray(mask) != 0) == bool(value)
    lab, _ = ndimage.label(sel, structure=np.ones((3, 3)) if connectivity == 8 else None)
    return roots_from_labels(lab)


def labels_from_roots(root):
    """root plane -> 0 for background, 1, 2, .. in the order of the components' first pixels"""
    flat = np.asarray(root).reshape(-1)
    rank = np.cumsum(flat == np.arange(flat.size))
    return np.where(flat >= 0, rank[np.maximum(flat, 0)], 0).astype(np.int32).reshape(np.asarray(root).shape)


# ---- the clean rules, restated on a labelling function ---------------------------------------------------------------------------------
def clean(mask, min_area=0, holes=False, islands=False, largest=False, connectivity=8, roots=roots_union_find):
    """vdr_op_mask_clean on one plane -> (out uint8 [H, W], changed, stats [5])"""
    cur = np.asarray(mask) != 0
    changed = 0
    if holes:                                      # components of the CLEAR pixels below min_area become set (border ones too)
        root, area, _ = roots(cur, connectivity, 0)
        a = area.reshape(-1)[np.maximum(root, 0)]
        fill = (root >= 0) & (a < min_area)
        changed |= int(fill.any())
        cur = cur | fill
    if islands or largest:
        root, area, n = roots(cur, connectivity, 1)
        if n:
            flat = area.reshape(-1)
            best = int(np.flatnonzero(flat == flat.max())[0])        # the largest; the lowest root on a tie
            a = flat[np.maximum(root, 0)]
            keep = (root == best) if largest else (root >= 0) & ((a >= min_area) | (root == best))
            changed |= 2 * int((keep != cur).any())
            cur = keep
    out = cur.astype(np.uint8)
    stats = np.zeros(5, dtype=np.int32)
    if cur.any():
        ys, xs = np.nonzero(cur)
        stats[:] = [cur.sum(), xs.min(), ys.min(), xs.max(), ys.max()]
    return out, changed, stats


# ---- designed planes -----------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """A one-pixel-wide path that fills the plane: every even row, joined alternately at the right and the left end"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    m = np.zeros((H, W), dtype=np.uint8)
    m[0] = 1
    m[:, 0::2] = 1
    return m


def rings(H, W):
    """Concentric one-pixel rings, every second distance from the border set: nested holes"""
    y, x = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d % 2 == 0).astype(np.uint8)


def designed(H, W):
    """name -> plane [H, W] uint8; the planes that need room are left out of a plane too small for them"""
    y, x = np.mgrid[0:H, 0:W]
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    c = np.zeros((H, W), np.uint8)
    c[0, 0] = c[0, W - 1] = c[H - 1, 0] = c[H - 1, W - 1] = 1
    out["corners"] = c
    out["checkerboard"] = ((x + y) & 1).astype(np.uint8)
    out["diagonal"] = (x == y).astype(np.uint8)
    out["antidiagonal"] = (x + y == min(H, W) - 1).astype(np.uint8)
    out["serpentine"] = serpentine(H, W)
    out["comb"] = comb(H, W)
    out["rings"] = rings(H, W)
    if H > T and W > T:                            # two pixels touching only diagonally across the four-tile corner
        a = np.zeros((H, W), np.uint8)
        a[T - 1, T - 1] = a[T, T] = 1
        b = np.zeros((H, W), np.uint8)
        b[T - 1, T] = b[T, T - 1] = 1
        out["corner_diag_main"], out["corner_diag_anti"] = a, b
    if H >= 5 and W >= 7:                          # two components of equal area and a smaller one: the lowest root wins
        e = np.zeros((H, W), np.uint8)
        e[H - 2:, 0:2] = 1
        e[0:2, W - 2:] = 1
        e[2, 3] = 1
        out["equal_areas"] = e
    return out


def bernoulli(H, W, p, seed):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8)
