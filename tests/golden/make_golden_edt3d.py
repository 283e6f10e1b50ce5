"""Writes edt3d_sp_*.npz: a handful of small mask volumes and the squared Euclidean distance transform
scipy.ndimage.distance_transform_edt(selected, sampling=spacing) (1.15.3) gives for them under an integer voxel spacing --
rint(d * d) as int64, for the set voxels without `outside` and with every axis outside (the volume padded by one non-selected
voxel all round, the frame cut off again) and for the clear voxels with z alone outside -- plus scipy's binary_dilation and
binary_erosion with the ellipsoid of 3 mm at that spacing read as millimetres / 2^-10 where it is one.  Masks are bit-packed
(np.packbits over the flattened volume).  Run from the repository root: python tests/golden/make_golden_edt3d.py"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt3d_ref as E3  # noqa: E402

Z, H, W = 6, 11, 17
MODES = ((1, 0), (1, 7), (0, 4))          # (value, outside)


def blobs(seed):
    rng = np.random.default_rng(seed)
    fine = ndimage.zoom(rng.standard_normal((3, 4, 5)), 4, order=1)[:Z, :H, :W]
    return (fine > 0.1).astype(np.uint8)


def volumes():
    zz, yy, xx = np.mgrid[0:Z, 0:H, 0:W]
    one = np.ones((Z, H, W), np.uint8)
    one[Z - 2, 1, 5] = 0
    return {
        "blobs": (blobs(11), (2560, 717, 717)),
        "ball": (((2 * (zz - 3)) ** 2 + (yy - 5) ** 2 + (xx - 8) ** 2 <= 25).astype(np.uint8), (1, 1, 1)),
        "bernoulli50": (E3.bernoulli((Z, H, W), 0.5, 50), (1, 2, 5)),
        "bernoulli95": (E3.bernoulli((Z, H, W), 0.95, 95), (3, 1, 1)),
        "one_clear": (one, (65535, 1, 300)),
    }


def main():
    assert scipy.__version__ == "1.15.3", scipy.__version__
    for name, (m, q) in volumes().items():
        out = dict(shape=np.array(m.shape, dtype=np.int32), spacing=np.array(q, dtype=np.int32), mask=np.packbits(m.reshape(-1) != 0),
                   scipy_version=np.array(scipy.__version__))
        for value, outside in MODES:
            out[f"d2_v{value}_o{outside}"] = E3.scipy_d2(m, q, value, outside)
        r2 = E3.radius2(3.0) if q == (2560, 717, 717) else 9 * max(q) ** 2 // 4
        out["r2"] = np.array(r2, dtype=np.int64)
        out["dilate"] = np.packbits(ndimage.binary_dilation(m != 0, E3.ellipsoid(q, r2, m.shape)).reshape(-1))
        out["erode"] = np.packbits(ndimage.binary_erosion(m != 0, E3.ellipsoid(q, r2, m.shape)).reshape(-1))
        path = os.path.join(HERE, f"edt3d_sp_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, m.shape, q, int(m.sum()), int(out["d2_v1_o7"].max()), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
