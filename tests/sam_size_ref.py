"""What the SAM-at-other-sizes tests share (TEST HELPER): the cases of tests/golden/sam_hf_resize.npz and the float64
definition of the rel-pos resampling with its half-ulp check (tests/test_sam_size_cpu.py, tests/test_sam_size_gpu.py,
tests/test_workspace_contract_gpu.py)."""
import os

import numpy as np
import torch

from oracle import sam_oracle as so


def golden_cases(golden_dir):
    """(native cfg, sized cfg, batch, wseed, xseed, wscale, expected out[:, :keep]) per case of sam_hf_resize.npz"""
    g = np.load(os.path.join(golden_dir, "sam_hf_resize.npz"), allow_pickle=False)
    out = []
    for n in range(int(g["n_cases"])):
        v = lambda k: g[f"c{n}_{k}"]  # noqa: E731
        mk = lambda img: so.SamCfg(int(img), 16, 3, int(v("dim")), int(v("heads")), int(v("layers")), int(v("ffn")),  # noqa: E731
                                   int(v("window")), tuple(int(i) for i in v("global_idx")), int(v("out_chans")), 1e-6)
        out.append((mk(v("native")), mk(v("side")), int(v("batch")), int(v("wseed")), int(v("xseed")), float(g["wscale"]),
                    torch.from_numpy(v("out"))))
    return out


def linear_def(t, L):
    """the definition written out in float64 numpy: src = max((i + 0.5) L0 / L - 0.5, 0), neighbours clamped at the last row"""
    t = t.double().numpy()
    L0 = t.shape[0]
    out = np.empty((L, t.shape[1]), dtype=np.float64)
    for i in range(L):
        src = max((i + 0.5) * (L0 / L) - 0.5, 0.0)
        i0 = min(int(src), L0 - 1)
        i1 = min(i0 + 1, L0 - 1)
        lam = src - i0
        out[i] = (1.0 - lam) * t[i0] + lam * t[i1]
    return out


def within_half_ulp(got, want64):
    """|got - want| <= half an fp32 ulp at want: got is the float64 value rounded to fp32 once.  (Two float64 evaluation
    orders of the same blend differ by ~1e-16 relative: 2^-29 of an fp32 ulp, allowed for by the 1e-6.)"""
    got = got.detach().cpu().double().numpy()
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return bool((np.abs(got - want64) <= 0.5 * ulp * (1 + 1e-6)).all())
