#!/usr/bin/env python3
"""Cost of the facet descriptors: the log-bin kernel alone, the same output composed from torch ops, the overlapping
im2col as the bandwidth yardstick, and extract_descriptors against dense_tokens on one handle.

    python tools/descriptor_bench.py [--steps K] [--warmup W] > profiles/descriptor_bench.txt

One process, one device.  JSON lines:
  kernel "log_bin": vdr_op_log_bin on a bf16 facet [B, gh*gw, C] (preallocated work and out; CUDA events around K calls):
      ms per call and TB/s of ALGORITHMIC bytes (input read once + output written once), h = 2 and 3, bf16 and fp32 out, for
      ViT-B/16 batch 64 at 224^2 with stride 16 (14 x 14) and stride 8 (27 x 27), and ViT-S/14 batch 16 (16 x 16);
      beside it "torch_ms": the same tensor from avg_pool2d(count_include_pad=False) + clamped index gather + cat on the
      same device, and the ratio torch_ms / ms.
  kernel "im2col": the stride-8 overlapping im2col of ViT-B/16 batch 64 (tools/patch_stride_bench.py's measurement), GB/s
      of algorithmic bytes -- the neighbouring write-bound kernel.
  workload lines: dense_tokens (bf16 out) against extract_descriptors(layer=last, facet="key") and its bin=True form on
      the same handle, ms per call (the key request stops after the last block's qkv GEMM)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from tools.patch_stride_bench import im2col_ms, timed  # noqa: E402


def bin_offsets(h):
    out = []
    for k in range(h):
        s = 3 ** k
        out += [(k, dy, dx) for dy in (-s, 0, s) for dx in (-s, 0, s) if not (k and dy == 0 and dx == 0)]
    return out


def torch_log_bin(x, gh, gw, h, out_dtype):
    """the upstream formulation on the device: fp32 pooling maps, clamped gathers, one cat"""
    B, n, C = x.shape
    f = x.float().reshape(B, gh, gw, C).permute(0, 3, 1, 2)
    maps = [f] + [torch.nn.functional.avg_pool2d(f, 3 ** k, 1, 3 ** k // 2, count_include_pad=False) for k in range(1, h)]
    ys0, xs0 = torch.arange(gh, device=x.device), torch.arange(gw, device=x.device)
    bins = []
    for k, dy, dx in bin_offsets(h):
        ys, xs = (ys0 + dy).clamp(0, gh - 1), (xs0 + dx).clamp(0, gw - 1)
        bins.append(maps[k][:, :, ys][:, :, :, xs].permute(0, 2, 3, 1))  # B, gh, gw, C
    return torch.cat(bins, dim=-1).reshape(B, n, len(bins) * C).to(out_dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import vdr
    from oracle import vit_oracle as vo
    from vdr import _lib as L
    torch.cuda.set_device(0)
    lib = L.load()
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup}), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    for name, B, gh, gw, C in (("vit_base16_224 stride 16", 64, 14, 14, 768), ("vit_base16_224 stride 8", 64, 27, 27, 768),
                               ("dinov2_small14 224^2", 16, 16, 16, 384)):
        n = gh * gw
        x = torch.randn(B, n, C, device="cuda").to(torch.bfloat16)
        for h in (2, 3):
            work = torch.empty((h - 1) * B * n * C, dtype=torch.float32, device="cuda")
            for dt in (torch.bfloat16, torch.float32):
                out = torch.empty((B, n, (1 + 8 * h) * C), dtype=dt, device="cuda")

                def run():
                    L.check(lib.vdr_op_log_bin(x.data_ptr(), L.VDR_BF16, C, n * C, B, gh, gw, C, h, work.data_ptr(), out.data_ptr(),
                                               L.VDR_BF16 if dt == torch.bfloat16 else L.VDR_F32, stream))
                ms = timed(run, args.steps, args.warmup)
                ref = torch_log_bin(x, gh, gw, h, dt)
                same = bool(torch.equal(out[:, :, :9 * C], ref[:, :, :9 * C]))
                maxerr = float((out.float() - ref.float()).abs().max())
                del ref
                tms = timed(lambda: torch_log_bin(x, gh, gw, h, dt), max(args.steps // 4, 3), 2)
                by = x.numel() * 2.0 + out.numel() * out.element_size()
                print(json.dumps({"kernel": "log_bin", "workload": name, "batch": B, "grid": [gh, gw], "C": C, "hierarchy": h,
                                  "out": "bf16" if dt == torch.bfloat16 else "fp32", "ms": round(ms, 4),
                                  "algorithmic_MB": round(by / 1e6, 1), "TB_per_s": round(by / ms / 1e9, 3), "torch_ms": round(tms, 4),
                                  "torch_over_kernel": round(tms / ms, 2), "level0_bitwise_torch": same, "max_abs_diff_torch": maxerr}),
                      flush=True)
                del out
                torch.cuda.empty_cache()
    # the yardstick and the whole forwards: ViT-B/16, batch 64, bf16 images
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    e = model.engine
    B, p = 64, cfg.patch
    xi = torch.rand(B, 3, 224, 224).to(torch.bfloat16).cuda()
    Kp = (3 * p * p + 63) // 64 * 64
    for s in (16, 8):
        e.set_patch_stride(s)
        if s != p:
            ms, per_fwd = im2col_ms(e, xi, args.steps, args.warmup)
            by = B * 3 * 224 * 224 * 2.0 + 2.0 * B * e.n_patches * Kp
            print(json.dumps({"kernel": "im2col", "workload": "vit_base16_224", "p": p, "stride": s, "pixels": "bf16", "batch": B,
                              "rows": B * e.n_patches, "Kp": Kp, "launches_per_forward": per_fwd, "ms": round(ms, 4),
                              "algorithmic_MB": round(by / 1e6, 2), "GB_per_s": round(by / ms / 1e6, 1)}), flush=True)
        last = cfg.layers - 1
        row = {"workload": "vit_base16_224", "stride": s, "grid": list(e.grid), "batch": B,
               "dense_tokens_ms": round(timed(lambda: model.dense_tokens(xi), args.steps, args.warmup), 3),
               "key_last_ms": round(timed(lambda: model.extract_descriptors(xi, last, "key"), args.steps, args.warmup), 3),
               "token_last_ms": round(timed(lambda: model.extract_descriptors(xi, last, "token"), args.steps, args.warmup), 3)}
        row["key_last_bin2_ms"] = round(timed(lambda: model.extract_descriptors(xi, last, "key", bin=True), args.steps, args.warmup), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
