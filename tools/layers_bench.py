#!/usr/bin/env python3
"""Step times of the intermediate-layer outputs (vdr_forward_layers) against the routes they replace.

    python tools/layers_bench.py [--steps K] [--warmup W]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/layers_bench.py --steps 5 --warmup 2   (per-kernel times)

ViT-B/16 224^2, batch 256, bf16 images (bench.py's workload):
  forward_features            vdr_forward, CLS out (the headline path)
  linear_probe_features(4)    one vdr_forward_layers call: CLS of blocks 8..11 + the pooled block 11, into [B, 5D]
  dense_mean                  the route pooling replaces: the [B, n, D] fp32 dense output, then torch.mean over n
  pooled_only                 vdr_forward_layers with the pooled block 11 alone
DINOv2-S/14 896^2 (n = 4096), batch 16: pooled_only and dense_mean.
Prints one JSON line per workload (ms per step = mean over K timed steps, CUDA events on the current stream)."""
import argparse
import json
import os
import sys

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
    for name, cfg, B, full in (("vit_base16_224", vo.VitCfg(), 256, True),
                               ("dinov2_small14_896", vo.VitCfg(896, 14, 3, 384, 6, 12, 1536, layerscale=True), 16, False)):
        w = vo.make_weights(cfg, seed=1, scale=0.02)
        x = vo.make_images(cfg, B, seed=0).cuda().to(torch.bfloat16)
        vc = vdr.VdrConfig(img=cfg.img, patch=cfg.patch, dim=cfg.dim, heads=cfg.heads, layers=cfg.layers,
                           mlp_hidden=cfg.mlp_hidden, layerscale=cfg.layerscale)
        model = vdr.VitDescriptorModel(vc, w)
        e, L, D = model.engine, cfg.layers, cfg.dim
        pooled = torch.empty((B, D), device="cuda")
        res = {"workload": name, "batch": B, "n_patches": cfg.n_patches, "dim": D}
        res["pooled_only_ms"] = timed(lambda: e.forward_layers(x, [vdr.LayerOut(L - 1, vdr.OUT_POOLED, out=pooled)]),
                                      args.steps, args.warmup)
        res["dense_mean_ms"] = timed(lambda: e.forward(x, vdr.OUT_DENSE, torch.float32).mean(dim=1), args.steps, args.warmup)
        if full:
            res["forward_features_ms"] = timed(lambda: model.forward_features(x), args.steps, args.warmup)
            res["linear_probe_features_ms"] = timed(lambda: model.linear_probe_features(x, 4), args.steps, args.warmup)
        res["pooled_bytes_read"] = B * cfg.n_patches * D * 2
        print(json.dumps(res), flush=True)
        del model, e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
