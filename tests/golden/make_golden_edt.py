"""Writes edt_sp_*.npz: a handful of mask planes and the squared Euclidean distance transform scipy.ndimage.distance_transform_edt
(1.15.3) gives for them -- rint(d * d) as int32, for the set pixels (value 1) and for the clear pixels (value 0), without and
with `outside` (the plane padded by one non-selected pixel all round, the frame cut off again) -- plus scipy's binary_dilation
and binary_erosion with the Euclidean disc of radius 3.5.  Masks are bit-packed (np.packbits over the flattened plane).
Run from the repository root: python tests/golden/make_golden_edt.py"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt_ref as ER  # noqa: E402

RADIUS = 3.5


def blobs(H, W, seed):
    """SAM-like blobs: a coarse random field up-sampled bilinearly and thresholded"""
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((H // 8 + 2, W // 8 + 2))
    fine = ndimage.zoom(coarse, 8, order=1)[:H, :W]
    return (fine + 0.15 * rng.standard_normal((H, W)) > 0.3).astype(np.uint8)


def planes():
    H, W = 97, 131   # more than one 64 x 16 tile and more than one segment a lane in the row pass, no multiple of either
    yy, xx = np.mgrid[0:H, 0:W]
    one = np.ones((H, W), np.uint8)
    one[H - 2, 5] = 0
    return {
        "blobs": blobs(H, W, 11),
        "disc": ((yy - 50) ** 2 + (xx - 60) ** 2 <= 40 ** 2).astype(np.uint8),
        "bernoulli50": ER.bernoulli(H, W, 0.5, 50),
        "bernoulli99": ER.bernoulli(H, W, 0.99, 99),
        "one_clear": one,
        "diagonal": (np.abs(yy - xx * (H - 1) // (W - 1)) <= 0).astype(np.uint8),   # one pixel thin
    }


def main():
    assert scipy.__version__ == "1.15.3", scipy.__version__
    for name, m in planes().items():
        out = dict(shape=np.array(m.shape, dtype=np.int32), mask=np.packbits(m.reshape(-1) != 0), scipy_version=np.array(scipy.__version__))
        for value in (0, 1):
            for outside in (0, 1):
                out[f"d2_v{value}_o{outside}"] = ER.scipy_d2(m, value, bool(outside))
        out["dilate"] = np.packbits(ndimage.binary_dilation(m != 0, ER.disc(RADIUS)).reshape(-1))
        out["erode"] = np.packbits(ndimage.binary_erosion(m != 0, ER.disc(RADIUS)).reshape(-1))
        path = os.path.join(HERE, f"edt_sp_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, m.shape, int(m.sum()), int(out["d2_v1_o0"].max()), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
