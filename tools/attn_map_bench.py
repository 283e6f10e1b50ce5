#!/usr/bin/env python3
"""Cost of the attention maps (vdr_forward_attn_maps, csrc/attention_probs.hip) on bench.py's workload.

    python tools/attn_map_bench.py [--steps K] [--warmup W]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/attn_map_bench.py --steps 5 --warmup 2   (per-kernel times)

ViT-B/16 224^2, batch 256, bf16 images, seeded weights:
  forward_features      vdr_forward, CLS out (the headline step)
  cls_map_step          vdr_forward_attn_maps: the CLS feature of block 11 + the CLS-row map of block 11 (fp32)
  op cls_map            vdr_op_attention_probs alone on a [256*197, 2304] qkv: q_rows 1, per head, fp32
  op full_mean          q_rows 197, head_mean, fp32   ([256, 197, 197])
  op full_heads         q_rows 197, per head, fp32    ([256, 12, 197, 197]: 477 MB)
Prints one JSON line per workload: ms (mean over K timed steps, CUDA events on the current stream) and, for the ops, the
bytes the map writes and that store rate."""
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
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_map_bench needs the MI355X (no CPU path)")
    import vdr
    from vdr import ops
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg(224, 16, 3, 768, 12, 12, 3072)
    B, N, H, dh = args.batch, cfg.n_tokens, cfg.heads, cfg.dim // cfg.heads
    e = vdr.Engine(vdr.VdrConfig(img=224, patch=16, dim=768, heads=12, layers=12, mlp_hidden=3072))
    e.load_weights(vo.make_weights(cfg, seed=1))
    x = vo.make_images(cfg, B, seed=0).to(torch.bfloat16).cuda()
    L = cfg.layers - 1
    cls_out = torch.empty(B, cfg.dim, device="cuda")
    cls_map = torch.empty(B, H, 1, N, device="cuda")
    specs = [vdr.LayerOut(L, vdr.OUT_CLS, out=cls_out)]
    maps = [vdr.AttnMap(L, 1, out=cls_map)]
    rows = []
    t_step = timed(lambda: e.forward(x, vdr.OUT_CLS), args.steps, args.warmup)
    rows.append(dict(workload="forward_features", batch=B, ms=t_step))
    t_map_step = timed(lambda: e.forward_attn_maps(x, maps, specs), args.steps, args.warmup)
    rows.append(dict(workload="cls_map_step", batch=B, ms=t_map_step, vs_forward=t_map_step / t_step))
    gen = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * N, 3 * H * dh, generator=gen) * 0.5).to(torch.bfloat16).cuda()
    for name, q_rows, mean in (("cls_map", 1, False), ("full_mean", N, True), ("full_heads", N, False)):
        out_bytes = B * (1 if mean else H) * q_rows * N * 4
        t = timed(lambda: ops.attention_probs(qkv, B, N, H, dh, q_rows, mean), args.steps, args.warmup)
        rows.append(dict(workload=f"op {name}", batch=B, q_rows=q_rows, head_mean=mean, ms=t, out_bytes=out_bytes,
                         store_gbs=out_bytes / t / 1e6, share_of_step=t / t_step))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
