"""Generate tests/golden/kmeans_sk_*.npz (run ONCE in the authoring container; provenance and measured gates: README_kmeans.md).

    python tests/golden/make_golden_kmeans.py            # writes the three files, prints the figures of the README
    python tests/golden/make_golden_kmeans.py search     # how the seeds in MAPS were found: the first seed per map that passes

Planted-cluster maps (tests/kmeans_ref.py `planted`: k centres N(0, sep^2) per channel, rows = centre + N(0, 1), channel c
scaled by 1 / (1 + decay c), rounded to bf16 and stored as their 16 bits), an init of k distinct rows of the map drawn with the
map's seed, and sklearn.cluster.KMeans(n_clusters=k, init=<that init>, n_init=1, tol=0, max_iter=300, algorithm="lloyd") on
the float64 values:
    kmeans_sk_130x32.npz     130 x 32,  k = 3
    kmeans_sk_333x96.npz     333 x 96,  k = 7
    kmeans_sk_520x416.npz    520 x 416, k = 10
The separation is low enough that Lloyd needs at least 10 iterations.

Asserted here, because the comparison means nothing without it -- a seed passes only when all hold:
  1. at every iteration of the float64 restatement's trajectory (tests/kmeans_ref.py `lloyd`), every row's margin between its
     best and second-best h exceeds 4 x the restatement's label bound (`assign_bounds`): no fp32 evaluation of the definition
     can label a row differently, so the kernels' trajectory is the restatement's;
  2. no cluster ever empties;
  3. sklearn's labels equal the restatement's, and the fit took at least 10 iterations."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_ref as kr  # noqa: E402

#        name               R    d    k   sep   decay  seed
MAPS = (("kmeans_sk_130x32", 130, 32, 3, 0.35, 0.0, 4),
        ("kmeans_sk_333x96", 333, 96, 7, 0.30, 0.0, 1),
        ("kmeans_sk_520x416", 520, 416, 10, 0.30, 0.0, 45))   # seeds: the first that `search` finds


def attempt(R, d, k, sep, decay, seed):
    """-> (dict of what the npz holds, dict of figures) or (None, the reason)"""
    from sklearn.cluster import KMeans
    x, _ = kr.planted(R, d, k, sep, seed, decay)
    rng = np.random.default_rng(seed + 10_000)
    init = x[np.sort(rng.choice(R, k, replace=False))].astype(np.float32)
    worst = [np.inf]
    empties = [False]

    def step(it, a, c):
        lb, _, _ = kr.assign_bounds(x, c, a)
        worst[0] = min(worst[0], float((a["margin"] / lb).min()))
        empties[0] = empties[0] or len(np.unique(a["labels"])) < k

    ref = kr.lloyd(x, init, 300, step)
    if not ref["converged"] or ref["iters"] < 10:
        return None, f"iters {ref['iters']}"
    if empties[0]:
        return None, "a cluster emptied"
    if worst[0] <= 4.0:
        return None, f"margin / bound {worst[0]:.2f}"
    sk = KMeans(n_clusters=k, init=init.astype(np.float64), n_init=1, tol=0, max_iter=300, algorithm="lloyd").fit(x.astype(np.float64))
    if not (sk.labels_ == ref["labels"]).all():
        return None, "sklearn's labels differ"
    emu = kr.lloyd_fp32(x, init, 300)
    assert (emu["labels"] == ref["labels"]).all() and emu["iters"] == ref["iters"]
    cb = kr.centroid_bound(x, ref["labels"], ref["centroids"])
    figs = dict(seed=seed, iters=ref["iters"], sk_n_iter=int(sk.n_iter_), min_margin_over_bound=worst[0],
                centre_dist_ref=float(np.abs(ref["centroids"] - sk.cluster_centers_).max()),
                centre_dist_emu=float(np.abs(emu["centroids"].astype(np.float64) - sk.cluster_centers_).max()),
                centre_bound_min_slack=float((cb - np.abs(emu["centroids"].astype(np.float64) - sk.cluster_centers_)).min()),
                inertia_rel_ref=float(abs(ref["inertia"] - sk.inertia_) / sk.inertia_),
                inertia_rel_emu=float(abs(float(emu["inertia"]) - sk.inertia_) / sk.inertia_))
    data = dict(x_bits=kr.bf16_bits(x), init=init, sk_labels=sk.labels_.astype(np.int32), sk_centers=sk.cluster_centers_,
                sk_inertia=np.float64(sk.inertia_), sk_n_iter=np.int32(sk.n_iter_), ref_iters=np.int32(ref["iters"]),
                seed=np.int32(seed))
    return data, figs


def main():
    import sklearn
    print("sklearn", sklearn.__version__, "numpy", np.__version__)
    search = len(sys.argv) > 1 and sys.argv[1] == "search"
    for name, R, d, k, sep, decay, seed0 in MAPS:
        if search:
            for seed in range(2000):
                data, figs = attempt(R, d, k, sep, decay, seed)
                if data is not None:
                    print(name, figs)
                    break
            else:
                print(name, "no seed below 2000 passes")
            continue
        data, figs = attempt(R, d, k, sep, decay, seed0)
        assert data is not None, (name, figs)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **data)
        print(name, figs, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
