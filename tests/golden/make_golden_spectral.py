"""Regenerates tests/golden/spectral_sp_{130x32,333x96,520x416}.npz: planted three-cluster descriptor maps
(tests/spectral_ref.py: planted), their float64 affinity graph at tau = 0.2 and SciPy's dense generalised eigen-decomposition
of (D - W) y = lambda D y, W = eps + (1 - eps) B, eps = 1e-5.  Run from the repository root:
    python tests/golden/make_golden_spectral.py
Needs numpy, torch (bf16 rounding) and scipy (written with SciPy 1.15.3).  README_spectral.md describes the files."""
import os
import sys

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spectral_ref as sref  # noqa: E402

CASES = ((130, 32, (10, 13)), (333, 96, (9, 37)), (520, 416, (20, 26)))
SEED, TAU, EPS = 1, 0.2, 1e-5


def main():
    print("scipy", scipy.__version__)
    for t, d, grid in CASES:
        x, first, rounds = sref.planted(t, d, SEED, TAU)
        s = sref.similarity(x[None])
        b = sref.graph(x[None], TAU)[0]
        margin = np.abs(s - float(np.float32(TAU))) / sref.bound(x[None], s)
        margin[0][np.arange(t), np.arange(t)] = np.inf
        vals, vec = sref.fiedler_dense(b, EPS, 4)
        part, seed, mask, box = sref.tokencut(vec, grid)
        dev = np.abs(vec - vec.mean())
        bits16 = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
        assert np.array_equal(torch.from_numpy(bits16).view(torch.bfloat16).float().numpy(), x)
        np.savez_compressed(os.path.join(HERE, f"spectral_sp_{t}x{d}.npz"), x_bf16=bits16, graph=np.packbits(b, axis=1),
                            eigvals=vals, fiedler=vec, bipartition=part, seed=np.int64(seed), mask=mask, box=np.array(box, np.int64),
                            grid=np.array(grid, np.int64), tau=np.float64(TAU), eps=np.float64(EPS))
        print(f"{t} x {d}: {first} entries within 4 x bound on the first draw, cleared after {rounds} redraw rounds; min |s - tau| / bound "
              f"{margin.min():.2f}; edge share {b.mean():.3f}; lambda_1..4 {np.array2string(vals, precision=6)}; smallest "
              f"|f_i - mean| / max|f - mean| {dev.min() / dev.max():.4f}; bipartition holds {int(part.sum())} of {t}, seed {seed}, "
              f"box {box}; clusters in the bipartition {[int(part.reshape(-1)[c::3].sum()) for c in range(3)]}")


if __name__ == "__main__":
    main()
