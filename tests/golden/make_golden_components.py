"""Writes components_sp_*.npz: a handful of mask planes labelled by scipy.ndimage.label (1.15.3; structure = np.ones((3, 3)) for
connectivity 8, the default cross for 4), for the set pixels (value 1) and for the clear pixels (value 0), and cleaned by the
rules of vdr_op_mask_clean restated on top of scipy's labels and np.bincount (tests/components_ref.clean with
roots = scipy_roots).  Masks are bit-packed (np.packbits over the flattened plane), label planes stored as scipy returns them;
the tests take "the first index per label" as the root.  Run from the repository root: python tests/golden/make_golden_components.py"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_ref as CR  # noqa: E402

CLEAN_CASES = [  # (name, keywords of components_ref.clean)
    ("holes_islands_8", dict(min_area=12, holes=True, islands=True, connectivity=8)),
    ("holes_islands_4", dict(min_area=12, holes=True, islands=True, connectivity=4)),
    ("islands_all_below_8", dict(min_area=100000, islands=True, connectivity=8)),
    ("largest_4", dict(largest=True, connectivity=4)),
    ("holes_largest_8", dict(min_area=40, holes=True, largest=True, connectivity=8)),
]


def blobs(H, W, seed):
    """SAM-like blobs: a coarse random field up-sampled bilinearly and thresholded"""
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((H // 8 + 2, W // 8 + 2))
    fine = ndimage.zoom(coarse, 8, order=1)[:H, :W]
    return (fine + 0.15 * rng.standard_normal((H, W)) > 0.3).astype(np.uint8)


def planes():
    H, W = 97, 131   # more than one 64 x 64 tile in both directions, no multiple of it
    return {
        "bernoulli41": CR.bernoulli(H, W, 0.41, 41),
        "bernoulli59": CR.bernoulli(H, W, 0.59, 59),
        "rings": CR.rings(H, W),
        "serpentine": CR.serpentine(H, W),
        "blobs": blobs(H, W, 7),
    }


def main():
    assert scipy.__version__ == "1.15.3", scipy.__version__
    for name, m in planes().items():
        out = dict(shape=np.array(m.shape, dtype=np.int32), mask=np.packbits(m.reshape(-1) != 0), scipy_version=np.array(scipy.__version__))
        for conn in (4, 8):
            for value in (0, 1):
                lab, n = ndimage.label((m != 0) == bool(value), structure=np.ones((3, 3)) if conn == 8 else None)
                out[f"labels_c{conn}_v{value}"] = lab.astype(np.int32)
                out[f"count_c{conn}_v{value}"] = np.array(n, dtype=np.int32)
        for cname, kw in CLEAN_CASES:
            o, changed, stats = CR.clean(m, roots=CR.scipy_roots, **kw)
            out[f"clean_{cname}"] = np.packbits(o.reshape(-1) != 0)
            out[f"clean_{cname}_changed"] = np.array(changed, dtype=np.int32)
            out[f"clean_{cname}_stats"] = stats
        path = os.path.join(HERE, f"components_sp_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, m.shape, int(m.sum()), {k: int(out[k]) for k in out if k.startswith("count")}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
