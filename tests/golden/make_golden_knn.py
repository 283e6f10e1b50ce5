#!/usr/bin/env python
"""Writes tests/golden/knn_sk_300x700x64.npz, knn_sk_d256_k16.npz and README_knn.md: scikit-learn's brute-force neighbours and
k-NN classifier (float64) on planted-cluster data, for tests/test_knn_cpu.py.

Data: tests/knn_ref.py `planted` (7 centres, noise 0.5, every value rounded to bf16 first).  sklearn runs in float64:
NearestNeighbors(algorithm="brute", metric="euclidean" | "cosine").kneighbors and KNeighborsClassifier(weights="uniform")
.predict_proba / .predict.

Only queries whose first k + 1 neighbours are separated by more than the fp32 bounds of tests/knn_ref.py are kept
(knn_ref.clear_rows), so that a test may demand sklearn's indices EXACTLY from an fp32 evaluation:
  knn_sk_300x700x64.npz   700 candidates, d = 64, k = 5: the first 300 drawn queries clear for BOTH metrics
  knn_sk_d256_k16.npz     600 candidates, d = 256, k = 16: the first 128 drawn queries clear for each metric (two query sets)
Descriptors are stored as bf16 bit patterns (uint16).  Run from the repository root: python tests/golden/make_golden_knn.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.neighbors import KNeighborsClassifier, NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import knn_ref as kref  # noqa: E402

SK_METRIC = {"cosine": "cosine", "l2": "euclidean"}


def clear_mask(q, c, k, metric):
    s = kref.scores(q[None], c[None], metric)
    return kref.clear_rows(s, kref.bound(q[None], c[None], s, metric), k, metric)[0], s[0]


def sk_block(q, c, labels, k, metric, s):
    """sklearn's answers for the queries q, checked against the restatement's stable sort before they are stored"""
    qn, cn = q.double().numpy(), c.double().numpy()
    dist, idx = NearestNeighbors(n_neighbors=k, algorithm="brute", metric=SK_METRIC[metric]).fit(cn).kneighbors(qn)
    _, want = kref.topk(s, k, metric)
    assert np.array_equal(idx, want), metric  # (clear rows: sklearn's order IS the float64 stable sort)
    clf = KNeighborsClassifier(n_neighbors=k, algorithm="brute", metric=SK_METRIC[metric], weights="uniform").fit(cn, labels.numpy())
    return {f"dist_{metric}": dist, f"idx_{metric}": idx.astype(np.int32), f"proba_{metric}": clf.predict_proba(qn),
            f"pred_{metric}": clf.predict(qn).astype(np.int64)}


def main():
    notes = []
    # ---- file 1: one query set, clear for both metrics
    d, k, nc, pool, keep = 64, 5, 700, 400, 300
    c, lab = kref.planted(nc, d, seed=11)
    q, _ = kref.planted(pool, d, seed=12)
    masks, ss = zip(*(clear_mask(q, c, k, m) for m in kref.METRICS))
    both = masks[0] & masks[1]
    notes.append(f"d={d} k={k} candidates={nc}: clear share cosine {masks[0].mean():.3f}, l2 {masks[1].mean():.3f}, both {both.mean():.3f} of {pool}")
    sel = np.flatnonzero(both)[:keep]
    assert sel.size == keep, (sel.size, keep)
    out = {"c": kref.bf16_bits(c), "q": kref.bf16_bits(q[sel]), "labels": lab.numpy(), "k": np.int64(k)}
    for m, s in zip(kref.METRICS, ss):
        out.update(sk_block(q[sel], c, lab, k, m, s[sel]))
    np.savez_compressed(os.path.join(HERE, "knn_sk_300x700x64.npz"), **out)
    # ---- file 2: a query set per metric
    d, k, nc, pool, keep = 256, 16, 600, 4000, 128
    c, lab = kref.planted(nc, d, seed=21)
    q, _ = kref.planted(pool, d, seed=22)
    out = {"c": kref.bf16_bits(c), "labels": lab.numpy(), "k": np.int64(k)}
    for m in kref.METRICS:
        mask, s = clear_mask(q, c, k, m)
        notes.append(f"d={d} k={k} candidates={nc}: clear share {m} {mask.mean():.3f} of {pool}")
        sel = np.flatnonzero(mask)[:keep]
        assert sel.size == keep, (m, sel.size, keep)
        out[f"q_{m}"] = kref.bf16_bits(q[sel])
        out.update(sk_block(q[sel], c, lab, k, m, s[sel]))
    np.savez_compressed(os.path.join(HERE, "knn_sk_d256_k16.npz"), **out)
    with open(os.path.join(HERE, "README_knn.md"), "w") as f:
        f.write("# k-NN golden files\n\n"
                "Written by `tests/golden/make_golden_knn.py` (its docstring has the recipe) with "
                f"scikit-learn {sklearn.__version__}, numpy {np.__version__}; float64 throughout.\n\n"
                "* `knn_sk_300x700x64.npz`: `c` [700, 64] and `q` [300, 64] as bf16 bit patterns (uint16), `labels` [700] "
                "(the planted cluster of every candidate), `k` = 5; per metric (`cosine`, `l2`): `dist_*` [300, 5] (sklearn's "
                "distance: 1 - cosine, Euclidean), `idx_*` [300, 5] int32, `proba_*` [300, 7] and `pred_*` [300] of "
                "`KNeighborsClassifier(weights=\"uniform\")`.\n"
                "* `knn_sk_d256_k16.npz`: `c` [600, 256], `labels`, `k` = 16, and per metric its own queries `q_*` [128, 256] "
                "with the same four arrays.\n\n"
                "Every stored query is one whose first k + 1 neighbours (and the k-th against all later ones) are separated by "
                "more than the fp32 bounds of `tests/knn_ref.py`; on those sklearn's indices equal the float64 stable sort "
                "(asserted by the generator), so an fp32 evaluation of the definition must return them exactly.\n\nMeasured while generating:\n\n"
                + "".join(f"* {n}\n" for n in notes))
    print("\n".join(notes))


if __name__ == "__main__":
    main()
