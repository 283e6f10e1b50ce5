#!/usr/bin/env python3
"""Cost of a finer patch stride (vdr_set_patch_stride): whole forwards and the overlapping im2col kernel alone.

    python tools/patch_stride_bench.py [--steps K] [--warmup W]

One process, bf16 images, random weights, CLS out.
  ViT-B/16 at 224^2, batch 64: stride 16 (default path: the im2col-free gather) / 8 / 4
  ViT-S/14 with a 518^2 table (the geometry of a dinov2_vits14 checkpoint) at 224^2, batch 16: stride 14 / 7
Per (model, stride) one JSON line: tokens, set_patch_stride_ms (mean of 5 calls, each coming from another stride), ms per
step (mean over K timed steps, CUDA events on the current stream), img/s and tokens/s.
Then the kernel alone: the handle's built-in profiler (HIP events around each launch) times the "im2col" class of a
PATCH_EMBED forward, per pixel type: ms per forward and GB/s of ALGORITHMIC bytes (pixels read once + col written once),
beside the stride-p im2col of the same images (p = 16 at stride p: fp32 pixels only, bf16 pixels skip im2col altogether)."""
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


def im2col_ms(e, x, steps, warmup):
    """(ms per forward, launches per forward) of the im2col class in a PATCH_EMBED forward, or (None, 0) without one"""
    import vdr
    for _ in range(warmup):
        e.forward(x, vdr.OUT_PATCH_EMBED, torch.bfloat16)
    torch.cuda.synchronize()
    e.profile(True, ["im2col"])
    e.profile_read()
    for _ in range(steps):
        e.forward(x, vdr.OUT_PATCH_EMBED, torch.bfloat16)
    torch.cuda.synchronize()
    r = e.profile_read().get("im2col")
    e.profile(False)
    return (r["ms"] / steps, r["launches"] // steps) if r else (None, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import vdr
    from oracle import vit_oracle as vo
    torch.cuda.set_device(0)
    size = (224, 224)
    for name, cfg, B, strides in (("vit_base16_224", vo.VitCfg(), 64, [16, 8, 4]),
                                  ("dinov2_small14_518", vo.VitCfg(518, 14, 3, 384, 6, 12, 1536, layerscale=True), 16, [14, 7])):
        model = vdr.load_model(name, weights=vo.make_weights(cfg, seed=1, scale=0.02))
        e = model.engine
        e.set_input_size(*size)
        p = cfg.patch
        x = torch.rand(B, 3, *size).to(torch.bfloat16).cuda()
        out = torch.empty((B, cfg.dim), dtype=torch.float32, device="cuda")
        for s in strides:
            other = 2 if s != 2 else p  # (every timed call really changes the stride)
            t_set = 0.0
            for _ in range(5):
                e.set_patch_stride(other)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.set_patch_stride(s)
                torch.cuda.synchronize()
                t_set += (time.perf_counter() - t0) * 1e3 / 5
            ms = timed(lambda: e.forward_into(x, out, vdr.OUT_CLS), args.steps, args.warmup)
            print(json.dumps({"workload": name, "size": list(size), "stride": s, "grid": list(e.grid), "batch": B,
                              "tokens": e.n_tokens, "set_patch_stride_ms": round(t_set, 3), "ms_per_step": round(ms, 3),
                              "img_per_s": round(B / ms * 1e3, 1), "tokens_per_s": round(B * e.n_tokens / ms * 1e3)}), flush=True)
        # the im2col kernel alone, per pixel type
        Kp = (3 * p * p + 63) // 64 * 64
        for s in strides:
            e.set_patch_stride(s)
            for dt in (torch.bfloat16, torch.float32):
                xd = x.to(dt)
                ms, per_fwd = im2col_ms(e, xd, args.steps, args.warmup)
                row = {"kernel": "im2col", "workload": name, "p": p, "stride": s, "pixels": "bf16" if dt == torch.bfloat16 else "fp32",
                       "batch": B, "rows": B * e.n_patches, "Kp": Kp}
                if ms is None:
                    row["note"] = "no im2col launch: the patch GEMM gathers its operand from the images"
                else:
                    by = B * 3 * size[0] * size[1] * xd.element_size() + 2.0 * B * e.n_patches * Kp
                    row.update({"launches_per_forward": per_fwd, "ms": round(ms, 4), "algorithmic_MB": round(by / 1e6, 2),
                                "GB_per_s": round(by / ms / 1e6, 1)})
                print(json.dumps(row), flush=True)
        del model, e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
