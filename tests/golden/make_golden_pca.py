"""Generate tests/golden/pca_*.npz (run ONCE in the authoring container; provenance and measured gates: README_pca.md).

    python tests/golden/make_golden_pca.py sklearn                       # main interpreter: scikit-learn only
    <conda python> tests/golden/make_golden_pca.py reference <reference checkout>/src
                                                                         # the interpreter that has skimage: the reference's
                                                                         # OWN visualization_utils.pca_colorize (module imported)

numpy only (no torch), so both interpreters can run it.

sklearn part -- planted-spectrum maps x = G diag(s) V^T + noise + mean, G [n, 6] gaussian, s = 8, 4, 2, 1, .5, .25 (so the
eigenvalues fall by ~16 from one to the next), V orthonormal, noise sd 0.05:
    pca_sk_64x64.npz      n = 64,   d = 64,  fp32; channels 5 and 40 carry means of about +60 and -35 at unit scale
    pca_sk_196x768.npz    n = 196,  d = 768, fp32 (a ViT-B/16 token map; sklearn's default solver is the randomized one here)
    pca_sk_1024x256.npz   n = 1024, d = 256, bf16 values stored as their 16 bits (a quarter MedSAM map)
each with sklearn.decomposition.PCA(n_components=3) on the float64 map, svd_solver="full" and the default, followed by the
reference's min_max_scale.
reference part -- pca_ref_colorize.npz: a clearly bimodal 32 x 32 x 64 map and visualization_utils.pca_colorize of it with
remove_bg False and True, the Otsu threshold and the mask.  Its seed is one at which sklearn's two sign conventions (scores
before release 1.5, components since) agree on the three components.

Asserted here, because the comparison means nothing without it: the eigenvalue ratios l2/l1, l3/l2, l4/l3 of every map are
<= 0.6 (the leading three directions are well separated from each other and from the fourth), and in the remove_bg case
no first-channel value lies within 1e-3 of the Otsu threshold."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
S = np.array([8.0, 4.0, 2.0, 1.0, 0.5, 0.25])
REF_SEED = 33  # (reference part: see the sign-convention note there)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 value (ties to even), returned as fp32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def planted(n, d, seed, mean_scale=0.5, noise=0.05):
    rng = np.random.default_rng(seed)
    v, _ = np.linalg.qr(rng.standard_normal((d, 6)))
    x = rng.standard_normal((n, 6)) * S @ v.T + noise * rng.standard_normal((n, d)) + mean_scale * rng.standard_normal(d)
    return x


def min_max_scale(data):
    lo, hi = data.min(), data.max()
    return (data - lo) / (hi - lo) if hi != lo else data


def check_ratios(lam, what):
    r = lam[1:4] / lam[0:3]
    assert np.all(r <= 0.6), (what, r)
    return r


def sklearn_part():
    import sklearn
    from sklearn.decomposition import PCA
    cases = {}
    x = planted(64, 64, 1)
    x[:, 5] = 60.0 + np.random.default_rng(11).standard_normal(64)
    x[:, 40] = -35.0 + np.random.default_rng(12).standard_normal(64)
    cases["pca_sk_64x64"] = x.astype(np.float32)
    cases["pca_sk_196x768"] = planted(196, 768, 2).astype(np.float32)
    cases["pca_sk_1024x256"] = bf16_round(planted(1024, 256, 3).astype(np.float32))
    for name, x32 in cases.items():
        x64 = x32.astype(np.float64)
        full = PCA(n_components=4, svd_solver="full").fit(x64)
        ratios = check_ratios(full.explained_variance_, name)
        full3 = PCA(n_components=3, svd_solver="full").fit(x64)
        dflt = PCA(n_components=3).fit(x64)
        out = dict(components=full3.components_, explained_variance=full3.explained_variance_,
                   explained_variance_ratio=full3.explained_variance_ratio_, mean=full3.mean_,
                   rgb_full=min_max_scale(full3.transform(x64)), rgb_default=min_max_scale(dflt.transform(x64)),
                   eigen_ratios=ratios, default_solver=np.array(getattr(dflt, "_fit_svd_solver", "?")),
                   sklearn_version=np.array(sklearn.__version__))
        if name == "pca_sk_1024x256":
            out["x_bf16_bits"] = (x32.view(np.uint32) >> 16).astype(np.uint16)
        else:
            out["x"] = x32
        np.savez(os.path.join(HERE, name + ".npz"), **out)
        print(name, x32.shape, "eigen ratios", ratios, "default solver", out["default_solver"],
              "default vs full on the scaled map", np.abs(out["rgb_full"] - out["rgb_default"]).max())


def reference_part(src):
    sys.path.insert(0, src)
    import skimage
    import sklearn
    import visualization_utils as vu  # the reference's own module
    from skimage.filters import threshold_otsu
    from sklearn.decomposition import PCA
    seed = REF_SEED
    rng = np.random.default_rng(4)
    h = w = 32
    x = planted(h * w, 64, seed)
    v, _ = np.linalg.qr(rng.standard_normal((64, 1)))
    yy, xx = np.mgrid[0:h, 0:w]
    fg = ((yy - 15.5) ** 2 + (xx - 13.0) ** 2 < 81.0).reshape(-1)  # a disc of "foreground" rows, far away along one direction
    x = (x + np.where(fg, 40.0, -40.0)[:, None] * v[:, 0]).astype(np.float32)
    x64 = x.astype(np.float64)
    lam = PCA(n_components=4, svd_solver="full").fit(x64).explained_variance_
    ratios = check_ratios(lam, "pca_ref_colorize")
    # this interpreter's sklearn (0.24) fixes a component's sign by its scores (svd_flip, u_based_decision=True), releases
    # from 1.5 on -- and this library -- by the component's own largest entry.  The seed is one at which the two agree
    # on all three components, so one file serves both.
    comps = PCA(n_components=3).fit(x64).components_
    agree = comps[np.arange(3), np.abs(comps).argmax(axis=1)] > 0
    assert agree.all(), ("sign conventions disagree at this seed", seed, agree)
    rgb = vu.pca_colorize(x64.copy(), (h, w), remove_bg=False)
    ch0 = rgb[:, :, 0].copy()
    thresh = threshold_otsu(ch0)
    margin = np.abs(ch0 - thresh).min()
    assert margin > 1e-3, margin
    mask = ch0 > thresh
    assert 0 < mask.sum() < mask.size
    rgb_bg = vu.pca_colorize(x64.copy(), (h, w), remove_bg=True)
    np.savez(os.path.join(HERE, "pca_ref_colorize.npz"), x=x, rgb=rgb, rgb_remove_bg=rgb_bg, otsu_threshold=np.array(thresh),
             otsu_margin=np.array(margin), mask=mask, eigen_ratios=ratios, skimage_version=np.array(skimage.__version__),
             sklearn_version=np.array(sklearn.__version__))
    print("pca_ref_colorize", x.shape, "eigen ratios", ratios, "otsu", thresh, "margin", margin, "foreground", int(mask.sum()),
          "skimage", skimage.__version__, "sklearn", sklearn.__version__)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "sklearn":
        sklearn_part()
    elif len(sys.argv) >= 3 and sys.argv[1] == "reference":
        reference_part(sys.argv[2])
    else:
        sys.exit(__doc__)
