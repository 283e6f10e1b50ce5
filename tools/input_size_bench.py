#!/usr/bin/env python3
"""Cost of running a model away from its native input size (vdr_set_input_size).

    python tools/input_size_bench.py [--steps K] [--warmup W]

Per workload: the time of the set_input_size call itself (pos_embed resampling + one table allocation, load-time class) and
the forward throughput, bf16 images, CLS out.
  ViT-B/16 (native 224^2), batch 64: 224^2 (native: the loaded table), 448^2 (square: the im2col-free gathered patch path),
      224x448 (rectangular: im2col)
  ViT-S/14 with a 518^2 table (the geometry of a dinov2_vits14 checkpoint), batch 16: 224^2 and 896^2
Prints one JSON line per (model, size): set_input_size_ms (mean of 5 calls, each coming from another size), ms per step
(mean over K timed steps, CUDA events on the current stream), img/s and tokens/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import vdr
    from oracle import vit_oracle as vo
    torch.cuda.set_device(0)
    for name, cfg, B, sizes in (("vit_base16_224", vo.VitCfg(), 64, [(224, 224), (448, 448), (224, 448)]),
                                ("dinov2_small14_518", vo.VitCfg(518, 14, 3, 384, 6, 12, 1536, layerscale=True), 16,
                                 [(224, 224), (896, 896)])):
        model = vdr.load_model(name, weights=vo.make_weights(cfg, seed=1, scale=0.02))
        e = model.engine
        for H, W in sizes:
            other = (cfg.patch * 3, cfg.patch * 5)  # (every timed call really changes the size)
            t_set = 0.0
            for _ in range(5):
                e.set_input_size(*other)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.set_input_size(H, W)
                torch.cuda.synchronize()
                t_set += (time.perf_counter() - t0) * 1e3 / 5
            x = torch.rand(B, 3, H, W).to(torch.bfloat16).cuda()
            out = torch.empty((B, cfg.dim), dtype=torch.float32, device="cuda")
            ms = timed(lambda: e.forward_into(x, out, vdr.OUT_CLS), args.steps, args.warmup)
            print(json.dumps({"workload": name, "native": cfg.img, "size": [H, W], "batch": B, "tokens": e.n_tokens,
                              "set_input_size_ms": round(t_set, 3), "ms_per_step": round(ms, 3),
                              "img_per_s": round(B / ms * 1e3, 1), "tokens_per_s": round(B * e.n_tokens / ms * 1e3)}), flush=True)
        del model, e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
