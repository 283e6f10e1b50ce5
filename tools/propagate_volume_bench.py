#!/usr/bin/env python3
"""Cost of the multi-source window vote and of the volume sweep built on it.

Op level: vdr.ops.window_vote (csrc/window_vote.hip, one launch) against vdr.local.vote_window, the same definition in torch
ops on the device (a stable sort of every [S * W * W] row, a gather, k elementwise passes), same inputs: random cosines and
soft labels, k = 5, T = 0.1, one problem.  Every shape is checked before it is timed: idx, val and labels equal, the scores
of both inside the bound of tests/window_vote_ref.py against its float64 restatement; the worst error / bound of the kernel
is printed.

End to end on one ViT-B/16 handle, a volume of 64 slices at 224 x 224, patch stride 16 and 8:
VitDescriptorModel.propagate_volume(n_context=7, direction="up", index=0) against a loop of propagate_labels over the
adjacent slices, each step's hard labels the next step's source -- what the library could do before (one hard source; two
slices per forward).  The two do not compute the same thing; the line reports what each costs.

    python tools/propagate_volume_bench.py [--rounds R] [--e2e 0|1] > profiles/propagate_volume_bench.txt

One process, one device; the sides alternate round by round, device events around `steps` calls after a warm-up; medians
over the rounds (tools/correspondence_bench.py's `interleaved`).  JSON lines; a ratio above 1 is a win of the first side."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import window_vote_ref as wref  # noqa: E402  (tests/: the restatement and its bound)
from correspondence_bench import interleaved  # noqa: E402  (tools/ is on sys.path when this file is run as a script)

SHAPES = tuple((S, grid, 4, C) for grid in ((27, 27), (63, 63)) for S in (1, 8) for C in (2, 8))
K, T = 5, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e", type=int, default=1)
    args = ap.parse_args()
    import vdr
    from vdr import local, ops
    torch.cuda.set_device(0)
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds}), flush=True)
    worst = 0.0
    for S, grid, r, C in SHAPES:
        cost, src = wref.random_inputs(1, S, grid, r, C, seed=S + C + grid[0])
        want = wref.vote(cost, src, grid, K, "softmax", T)
        bnd = wref.bound(cost, src, grid, K, "softmax", T)
        cost, src = cost.cuda(), src.cuda()
        # ---- checked before it is timed
        got, ref = ops.window_vote(cost, src, grid, K, temperature=T), local.vote_window(cost, src, grid, K, temperature=T)
        for a, b, name in zip(got[1:], ref[1:], ("labels", "idx", "val")):
            assert torch.equal(a, b), f"{name} differs from vote_window"
        assert np.array_equal(got[2].cpu().numpy(), want[2]), "idx differs from the restatement"
        ratios = [float((np.abs(o[0].cpu().numpy() - want[0]) / bnd).max()) for o in (got, ref)]
        assert max(ratios) <= 1.0, ratios
        worst = max(worst, ratios[0])
        (ms, tms), (ms_min, tms_min), steps = interleaved(
            [lambda: ops.window_vote(cost, src, grid, K, temperature=T), lambda: local.vote_window(cost, src, grid, K, temperature=T)],
            args.rounds)
        W = 2 * r + 1
        print(json.dumps({"kernel": "window_vote", "sources": S, "grid": list(grid), "radius": r, "k": K, "classes": C,
                          "row_floats": S * W * W, "cost_MB": round(S * grid[0] * grid[1] * W * W * 4 / 1e6, 2),
                          "ms": round(ms, 4), "ms_min": round(ms_min, 4), "torch_vote_window_ms": round(tms, 4),
                          "torch_vote_window_ms_min": round(tms_min, 4), "torch_over_kernel": round(tms / ms, 2),
                          "cost_GB_per_s": round(S * grid[0] * grid[1] * W * W * 4 / (ms * 1e-3) / 1e9, 1),
                          "error_over_bound_kernel": round(ratios[0], 3), "error_over_bound_torch": round(ratios[1], 3),
                          "steps_per_round": steps}), flush=True)
    print(json.dumps({"worst_error_over_bound_of_the_kernel": round(worst, 3)}), flush=True)
    if not args.e2e:
        return
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    Z, n_classes = 64, 4
    for stride in (16, 8):
        model.set_input_size(224, 224)
        model.set_patch_stride(stride)
        grid = tuple(model.grid)
        x = torch.rand(Z, 3, 224, 224).to(torch.bfloat16).cuda()
        labels = torch.randint(0, n_classes, grid, device="cuda")

        def loop_of_propagate_labels():
            lab = labels[None]
            for z in range(1, Z):
                lab = model.propagate_labels(x[z - 1:z], lab, x[z:z + 1], n_classes, radius=4, k=K).labels
            return lab

        def volume():
            return model.propagate_volume(x, labels, n_classes, index=0, radius=4, k=K, n_context=7, direction="up")

        def volume_one_source():
            return model.propagate_volume(x, labels, n_classes, index=0, radius=4, k=K, n_context=0, direction="up")

        (vol, one, loop), _, steps = interleaved([volume, volume_one_source, loop_of_propagate_labels], args.rounds, budget_ms=1000.0)
        print(json.dumps({"workload": "vit_base16 volume", "slices": Z, "size": 224, "stride": stride, "grid": list(grid),
                          "propagate_volume_n_context7_ms": round(vol, 2), "propagate_volume_n_context0_ms": round(one, 2),
                          "loop_of_propagate_labels_ms": round(loop, 2), "loop_over_volume": round(loop / vol, 3),
                          "loop_over_volume_one_source": round(loop / one, 3), "ms_per_slice_volume": round(vol / (Z - 1), 3),
                          "ms_per_slice_loop": round(loop / (Z - 1), 3), "steps_per_round": steps}), flush=True)


if __name__ == "__main__":
    main()
