"""Generate tests/golden/anomaly_sk_*.npz (run ONCE in the authoring container; provenance and measured gates:
README_anomaly.md).

    python tests/golden/make_golden_anomaly.py     # writes the files, prints the figures of the README

Planted-spectrum maps (tests/mahalanobis_ref.py `planted`: rows N(mu, Q diag(s) Q^T), s log-spaced from 1 to 1 / cond, rounded
to bf16 and stored as 16-bit patterns).  Per map NAME: NAME.npz holds the training rows, the test rows (inliers, then the
planted outliers) and scikit-learn's results -- EmpiricalCovariance / ShrunkCovariance(shrinkage=0.01) location_ and the
mahalanobis() of the test rows under each; NAME_cov.npz holds the two covariance_ matrices in float64 as upper triangles (a
file of its own so that each stays under 1 MB).  One per-position case (PaDiM): a 2 x 3 grid, 40 training images, d = 32, one
ShrunkCovariance per position.

The generator asserts that scikit-learn's own distances put every planted outlier at least 2 x above the largest inlier: the
ranking tests of tests/test_anomaly_gpu.py rest on this."""
import os
import sys

import numpy as np
import sklearn
from sklearn.covariance import EmpiricalCovariance, ShrunkCovariance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mahalanobis_ref as mr  # noqa: E402

SHRINKAGE = 0.01
#        name                  train  d    cond  test  outliers  seed
MAPS = (("anomaly_sk_600x32",   600,  32,  1e2,  96,   16,       11),
        ("anomaly_sk_1200x96",  1200, 96,  4e2,  96,   16,       12),
        ("anomaly_sk_1000x256", 1000, 256, 5e2,  96,   16,       13))
POS = ("anomaly_sk_pos_2x3x40x32", (2, 3), 40, 32, 1e1, 8, 2, 40)  # name, grid, images, d, cond, test images, outlier images, seed


def triu(a):
    return a[np.triu_indices(a.shape[0])]


def fit(train, test):
    res = {}
    for tag, est in (("emp", EmpiricalCovariance()), ("shr", ShrunkCovariance(shrinkage=SHRINKAGE))):
        est.fit(train.astype(np.float64))
        res[tag] = (est.location_.copy(), est.covariance_.copy(), est.mahalanobis(test.astype(np.float64)))
    return res


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name, n, d, cond, nt, nout, seed in MAPS:
        x, out = mr.planted(n + nt, d, cond, seed, n_out=nout)
        train, test, out = x[:n], x[n:], out[n:]
        r = fit(train, test)
        for tag in ("emp", "shr"):
            d2 = r[tag][2]
            ratio = d2[out].min() / d2[~out].max()
            print(f"{name} {tag}: largest inlier {d2[~out].max():.1f}, smallest outlier {d2[out].min():.1f}, ratio {ratio:.2f}")
            assert ratio >= 2.0
        assert np.array_equal(r["emp"][0], r["shr"][0])
        np.savez(os.path.join(HERE, name + ".npz"), train_bits=mr.bf16_bits(train), test_bits=mr.bf16_bits(test), is_outlier=out,
                 location=r["emp"][0], emp_d2=r["emp"][2], shr_d2=r["shr"][2], shrinkage=np.float64(SHRINKAGE))
        np.savez(os.path.join(HERE, name + "_cov.npz"), emp_cov_triu=triu(r["emp"][1]), shr_cov_triu=triu(r["shr"][1]))
    name, (gh, gw), imgs, d, cond, nt, nout, seed = POS
    t = gh * gw
    train = np.empty((imgs, t, d), np.float32)
    test = np.empty((nt, t, d), np.float32)
    loc = np.empty((t, d))
    cov = np.empty((t, d, d))
    d2 = np.empty((nt, t))
    for p in range(t):
        x, out = mr.planted(imgs + nt, d, cond, seed + p, n_out=nout)
        train[:, p], test[:, p] = x[:imgs], x[imgs:]
        r = fit(train[:, p], test[:, p])["shr"]
        loc[p], cov[p], d2[:, p] = r
    out = np.zeros((nt, t), bool)
    out[nt - nout:] = True
    ratio = d2[out].min() / d2[~out].max()
    print(f"{name}: largest inlier {d2[~out].max():.1f}, smallest outlier {d2[out].min():.1f}, ratio {ratio:.2f}")
    assert ratio >= 2.0
    np.savez(os.path.join(HERE, name + ".npz"), train_bits=mr.bf16_bits(train), test_bits=mr.bf16_bits(test), is_outlier=out,
             location=loc, shr_cov=cov, shr_d2=d2, shrinkage=np.float64(SHRINKAGE), grid=np.array([gh, gw]))
    for f in sorted(os.listdir(HERE)):
        if f.startswith("anomaly_sk_"):
            size = os.path.getsize(os.path.join(HERE, f))
            print(f"{f}: {size} bytes")
            assert size < 1000000


if __name__ == "__main__":
    main()
