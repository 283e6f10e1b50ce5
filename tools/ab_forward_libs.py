#!/usr/bin/env python3
"""Whole-forward A/B of two builds of libvdr.so in ONE process, interleaved rounds on one device (as tools/ab_libs.py does
for single kernels): both libraries are dlopen'ed side by side, each gets its own handle with the same weights, and the
headline forward (bench.py's workload: ViT-B/16 224^2, batch 256, bf16 images, CLS out) alternates between them.
   python tools/ab_forward_libs.py path/to/libA.so path/to/libB.so [--model vit_base16_224] [--batch 256] [--rounds 15] [--steps 10] [--fp8]
--model medsam: the SAM ViT-B image encoder at 1024^2 (neck output) instead of a plain ViT's CLS features.
--fp8: qkv / fc1 / fc2 as MX-fp8 (vdr_config.fp8 = 1).
Prints per library the median / min / max ms per step over the rounds, the per-round A - B differences, and whether the
median difference lies inside the round-to-round spread of either side.  The outputs of the two must be bitwise equal."""
import argparse
import ctypes as C
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
import torch  # noqa: E402

import vdr  # noqa: E402
from oracle import vit_oracle as vo  # noqa: E402  (weight generator only)
from vdr import _lib as L  # noqa: E402
from vdr.engine import Engine  # noqa: E402


def engine_on(path, cfg, weights):
    """An Engine whose calls go to the library at `path` (symbols an older build lacks stay unbound)."""
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in L.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    e = Engine.__new__(Engine)
    e.lib, e.cfg, e.device, e._ws, e._loaded = lib, cfg, torch.device("cuda", torch.cuda.current_device()), None, False
    h, cc = C.c_void_p(), cfg.to_c()
    rc = lib.vdr_create(C.byref(cc), e.device.index, C.byref(h))
    assert rc == 0, (path, rc, lib.vdr_last_error(None))
    e.h = h
    e.load_weights(weights)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--model", default="vit_base16_224")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--fp8", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sam = a.model == "medsam"
    if sam:
        from oracle import sam_oracle as so
        cfg = so.SAM_VIT_B
        w = so.make_weights(cfg, seed=1)
    else:
        cfg = vo.CONFIGS[a.model]
        w = vo.make_weights(cfg, seed=1)
    mode = vdr.OUT_ENCODER if sam else vdr.OUT_CLS
    arch = dataclasses.replace(vdr.ARCHS[a.model], fp8=1) if a.fp8 else vdr.ARCHS[a.model]
    engines = [engine_on(p, arch, w) for p in a.libs]
    x = torch.rand(a.batch, 3, cfg.img, cfg.img).to(torch.bfloat16).cuda()
    shape = (a.batch, cfg.grid, cfg.grid, cfg.out_chans) if sam else (a.batch, cfg.dim)
    outs = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in engines]
    times = [[] for _ in engines]
    for rnd in range(a.rounds + 1):
        order = [0, 1] if rnd & 1 else [1, 0]  # alternate who goes first
        for i in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            engines[i].forward_into(x, outs[i], mode)
            e0.record()
            for _ in range(a.steps):
                engines[i].forward_into(x, outs[i], mode)
            e1.record()
            torch.cuda.synchronize()
            if rnd:  # round 0 warms up
                times[i].append(e0.elapsed_time(e1) / a.steps)
    print(f"{a.model}{' MX-fp8' if a.fp8 else ''} batch {a.batch} bf16 images, {'neck' if sam else 'CLS'} out; {a.rounds} interleaved rounds of {a.steps} steps")
    print("outputs bitwise equal:", torch.equal(outs[0], outs[1]))
    med = []
    for p, t in zip(a.libs, times):
        s = sorted(t)
        med.append(s[len(s) // 2])
        print(f"{'AB'[len(med) - 1]} {p}: median {med[-1]:7.3f} ms/step  min {s[0]:7.3f}  max {s[-1]:7.3f}  spread {s[-1] - s[0]:6.3f}"
              f"  -> {a.batch / med[-1] * 1e3:8.1f} img/s", flush=True)
    print("per round A - B (ms):", " ".join(f"{p - q:+.3f}" for p, q in zip(*times)))
    spread = max(max(t) - min(t) for t in times)
    d = med[0] - med[1]
    print(f"median A - B = {d:+.3f} ms ({d / med[1] * 100:+.2f} %); round-to-round spread {spread:.3f} ms ->",
          "inside the spread" if abs(d) <= spread else "OUTSIDE the spread")


if __name__ == "__main__":
    main()
