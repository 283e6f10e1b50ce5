#!/usr/bin/env python3
"""Cost of the windowed correlation: vdr_op_local_correlation (row norms, the tile kernel, the fold over the window: cost and
best pair both asked for) against what a user runs without it --
  * this checkout's global match vdr.ops.nn_cosine(mutual=False) on the same inputs, and
  * the same cost volume from torch ops: a loop over the W * W offsets, each a shifted multiply and a sum over the channels
    (fp32 accumulation) of the L2-normalised bf16 maps
-- and, end to end on one ViT-B/16 handle, find_correspondences(radius=4) beside radius=None and propagate_labels beside
extract_descriptors plus the torch loop.  (torch's batched bf16 bmm is no yardstick here: profiles/correspondence_bench.txt
records wrong results from it at 8 x 3969 on this build.)

    python tools/local_correlation_bench.py [--rounds R] [--e2e 0|1] > profiles/local_correlation_bench.txt

One process, one device; the sides alternate round by round (who goes first alternates too), device events around `steps`
calls after a warm-up; medians over the rounds.  Every shape is checked before it is timed: the cost volume against the torch
loop (the same -inf slots; finite entries within 2e-2, the rounding of the normalised bf16 maps), the best pair against
nn_cosine bit for bit on the rows whose global match lies inside the window.  JSON lines:
  kernel "local_correlation": pairs, grid, d, radius, ms and the yardsticks' ms and ratios (yardstick / kernel: above 1 is a
      win), the tile work actually executed (items * 128 * 128 * d * 2 FLOP) over the kernel's time as TF/s and as a share of the
      2.5 PF dense bf16 peak, the share of that work that is in-window, and the global match's tile steps over the window's.
  workload lines: ms per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from correspondence_bench import interleaved  # noqa: E402  (tools/ is on sys.path when this file is run as a script)

PEAK_BF16 = 2.5e15
PH, PW = 8, 16  # the panel of csrc/local_corr_map.h

SHAPES = ((64, (14, 14), 768, 2), (32, (27, 27), 768, 4), (1, (63, 63), 768, 4), (8, (63, 63), 768, 4), (1, (63, 63), 768, 8),
          (8, (63, 63), 768, 8), (1, (63, 63), 13056, 4))


def torch_cost(x, y, grid, r):
    """the cost volume from torch ops: [P, t, W * W] fp32, -inf outside the grid"""
    gh, gw = grid
    P, t, d = x.shape
    W = 2 * r + 1
    xn = torch.nn.functional.normalize(x.float(), dim=-1).to(torch.bfloat16).view(P, gh, gw, d)
    yn = torch.nn.functional.normalize(y.float(), dim=-1).to(torch.bfloat16).view(P, gh, gw, d)
    cost = torch.full((P, gh, gw, W * W), float("-inf"), dtype=torch.float32, device=x.device)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy), min(gh, gh - dy), max(0, -dx), min(gw, gw - dx)
            if y0 < y1 and x0 < x1:
                cost[:, y0:y1, x0:x1, (dy + r) * W + dx + r] = \
                    (xn[:, y0:y1, x0:x1] * yn[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]).sum(-1, dtype=torch.float32)
    return cost.view(P, t, W * W)


def tile_counts(grid, r):
    gh, gw = grid
    panels = ((gh + PH - 1) // PH) * ((gw + PW - 1) // PW)
    tiles = ((PH + 2 * r) * (PW + 2 * r) + 127) // 128
    t = gh * gw
    return panels * tiles, ((t + 127) // 128) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e", type=int, default=1)
    args = ap.parse_args()
    import vdr
    from vdr import local, ops
    torch.cuda.set_device(0)
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds}), flush=True)
    for P, grid, d, r in SHAPES:
        t = grid[0] * grid[1]
        gen = torch.Generator(device="cuda").manual_seed(t + d + r)
        x = torch.randn(P, t, d, device="cuda", generator=gen).to(torch.bfloat16)
        y = torch.randn(P, t, d, device="cuda", generator=gen).to(torch.bfloat16)
        # ---- checked before it is timed
        cost, bs, bi = ops.local_correlation(x, y, grid, r)
        ref = torch_cost(x, y, grid, r)
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(cost), fin), "the -inf slots differ from the torch loop's"
        diff = float((cost[fin] - ref[fin]).abs().max())
        assert diff < 2e-2, diff
        rs, ri, _, _ = ops.nn_cosine(x, y, mutual=False)
        i = torch.arange(t, device="cuda").unsqueeze(0)
        inside = ((ri // grid[1] - i // grid[1]).abs() <= r) & ((ri % grid[1] - i % grid[1]).abs() <= r)
        assert torch.equal(bs[inside], rs[inside]) and torch.equal(bi[inside], ri[inside]), "best pair differs from nn_cosine inside the window"
        del ref, fin, cost
        (ms, gms, tms), (ms_min, gms_min, tms_min), steps = interleaved(
            [lambda: ops.local_correlation(x, y, grid, r), lambda: ops.nn_cosine(x, y, mutual=False), lambda: torch_cost(x, y, grid, r)],
            args.rounds)
        items, global_tiles = tile_counts(grid, r)
        flop = 2.0 * P * items * 128 * 128 * d
        W = 2 * r + 1
        useful = sum((grid[0] - abs(dy)) * (grid[1] - abs(dx)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
                     if abs(dy) < grid[0] and abs(dx) < grid[1])
        print(json.dumps({"kernel": "local_correlation", "pairs": P, "grid": list(grid), "t": t, "d": d, "radius": r, "slots": W * W,
                          "ms": round(ms, 4), "ms_min": round(ms_min, 4),
                          "nn_cosine_ms": round(gms, 4), "nn_cosine_ms_min": round(gms_min, 4), "nn_cosine_over_kernel": round(gms / ms, 3),
                          "torch_loop_ms": round(tms, 4), "torch_loop_ms_min": round(tms_min, 4), "torch_loop_over_kernel": round(tms / ms, 3),
                          "items_per_pair": items, "global_tiles_over_window_tiles": round(global_tiles / items, 2),
                          "executed_TF_per_s": round(flop / ms / 1e9, 1), "share_of_bf16_peak": round(flop / (ms * 1e-3) / PEAK_BF16, 4),
                          "in_window_share_of_executed": round(useful / (items * 128.0 * 128.0), 4),
                          "cost_MB": round(P * t * W * W * 4 / 1e6, 1), "steps_per_round": steps,
                          "max_abs_diff_to_torch_loop": diff, "share_of_rows_whose_global_match_is_in_window": round(float(inside.float().mean()), 4)}),
              flush=True)
        del x, y
        torch.cuda.empty_cache()
    if not args.e2e:
        return
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for size, stride, B in ((224, 16, 8), (224, 8, 8)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        grid = tuple(model.grid)
        x1 = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        x2 = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        labels = torch.randint(0, 4, (B,) + grid, device="cuda")

        def by_hand():
            d = model.extract_descriptors(torch.cat([x2, x1]), None, "key")[:, 0]
            return torch_cost(d[:B], d[B:], grid, 4)

        (loc, glob, prop, hand), _, steps = interleaved(
            [lambda: model.find_correspondences(x1, x2, radius=4), lambda: model.find_correspondences(x1, x2),
             lambda: model.propagate_labels(x1, labels, x2, 4, radius=4, k=5), by_hand], args.rounds)
        print(json.dumps({"workload": "vit_base16", "size": size, "stride": stride, "grid": list(grid), "pairs": B,
                          "find_correspondences_radius4_ms": round(loc, 3), "find_correspondences_global_ms": round(glob, 3),
                          "global_over_radius4": round(glob / loc, 3), "propagate_labels_radius4_k5_ms": round(prop, 3),
                          "extract_descriptors_plus_torch_loop_ms": round(hand, 3), "by_hand_over_propagate_labels": round(hand / prop, 3),
                          "steps_per_round": steps}), flush=True)


if __name__ == "__main__":
    main()
