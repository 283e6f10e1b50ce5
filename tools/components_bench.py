#!/usr/bin/env python3
"""Connected components of mask planes on one MI355X: what labelling and small-region removal cost, by content.

   python tools/components_bench.py [--rounds 5] [--steps 5] [--out profiles/components_bench.txt] [--no-end-to-end]
   python tools/components_bench.py --passes blobs|bernoulli|serpentine     (a few calls only: the run rocprofv3 traces)
   python tools/components_bench.py --kernel-stats DIR --out FILE            (appends the per-kernel times of traced runs)

* connected_components and mask_clean(holes + islands, min_area 100) at 1, 64 and 192 planes of 1024^2 and 192 planes of 256^2, on
  (a) SAM-like blobs (random low-resolution logits, up-sampled and thresholded), (b) Bernoulli(0.59) planes at connectivity 4 (near
  the lattice's percolation threshold: large, tortuous components), (c) the serpentine (one one-pixel-wide path through every seam).
  Outputs are checked first (against scipy on a plane, and area / count identities on all).
* yardsticks: scipy.ndimage.label + np.bincount on the host INCLUDING the device-to-host copy of the masks (measured on at most 8
  planes and scaled: it is linear in the planes), and vdr.components.label_torch on the device (one plane: it synchronises per round).
* algorithmic bytes / s: the mask read once (1 byte a pixel), the root written once (4 bytes a pixel).
* end to end: generate_masks with and without min_mask_region_area; the labelling step of TokenCut on the host and on the device.
Interleaved medians with min and max; losses are printed as losses."""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vdr  # noqa: E402
from segment_bench import interleaved  # noqa: E402
from vdr import components as cc, ops  # noqa: E402

CONTENTS = ("blobs", "bernoulli", "serpentine")
CONN = {"blobs": 8, "bernoulli": 4, "serpentine": 8}


def planes(kind, P, side, dev):
    g = torch.Generator(device="cpu").manual_seed(3)
    if kind == "blobs":
        low = torch.randn((P, 1, side // 16, side // 16), generator=g) * 3
        return (F.interpolate(low.to(dev), size=(side, side), mode="bilinear", align_corners=False)[:, 0] > 1.0).to(torch.uint8)
    if kind == "bernoulli":
        return (torch.rand((P, side, side), device=dev) < 0.59).to(torch.uint8)
    m = torch.zeros((side, side), dtype=torch.uint8, device=dev)
    m[0::2] = 1
    ys = torch.arange(1, side, 2, device=dev)
    m[ys, torch.where((torch.arange(ys.numel(), device=dev) % 2) == 0, side - 1, 0)] = 1
    return m[None].expand(P, -1, -1).contiguous()


def scipy_label(mask_dev, conn):
    """what a user without the op pays: the copy to the host, scipy's label, bincount for the areas"""
    from scipy import ndimage
    m = mask_dev.cpu().numpy()
    st = np.ones((3, 3)) if conn == 8 else None
    out = []
    for p in range(m.shape[0]):
        lab, n = ndimage.label(m[p], structure=st)
        out.append((lab, np.bincount(lab.reshape(-1), minlength=n + 1)))
    return out


def check(mask, conn):
    root, area, count = ops.connected_components(mask, conn)
    assert torch.equal(area.sum(dim=(1, 2)), (mask != 0).sum(dim=(1, 2))) and torch.equal((area != 0).sum(dim=(1, 2)).to(torch.int32), count)
    lab, cnt = scipy_label(mask[:1], conn)[0]
    assert np.array_equal(cc.relabel(root[:1]).cpu().numpy()[0], lab) and int(count[0]) == cnt.shape[0] - 1
    out, changed, stats = ops.mask_clean(mask, 100, holes=True, islands=True, connectivity=conn)
    assert torch.equal(stats[:, 0].long(), out.sum(dim=(1, 2)))
    return int(count[0]), int(area[0].max()), int(changed[0])


def passes(kind):
    dev = torch.device("cuda", 0)
    m = planes(kind, 64, 1024, dev)
    for _ in range(5):
        ops.connected_components(m, CONN[kind])
        ops.mask_clean(m, 100, holes=True, islands=True, connectivity=CONN[kind])
    torch.cuda.synchronize()


def kernel_stats(directory, out):
    """the cc_* rows of every traced --passes run under `directory` (rocprofv3's rocpd database, or its kernel_stats.csv where it
    wrote one), appended to `out`"""
    import re
    import sqlite3
    lines = ["per-pass times from rocprofv3 --kernel-trace --stats (a run of its own per content: 64 planes of 1024^2, 5 connected_components and "
             "5 mask_clean(holes + islands) calls; a labelling = tile + seam + flatten, mask_clean runs two labellings and two apply passes)"]

    def row(name, calls, total_ns, share):
        short = re.search(r"(cc_\w+_kernel|mask_binarize_kernel)", name)
        if short:
            lines.append(f"    {short.group(1):22s} calls {int(calls):4d}  total {float(total_ns) / 1e6:9.3f} ms  average {float(total_ns) / int(calls) / 1e3:8.1f} us  "
                         f"{float(share):5.1f} % of the run's kernel time")
    for f in sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)):
        lines.append(f"  {os.path.basename(os.path.dirname(f))}")
        rows = sqlite3.connect(f).execute("select name, count(*), sum(end - start) from kernels group by name order by 3 desc").fetchall()
        total = sum(r[2] for r in rows)
        for name, calls, ns in rows:
            row(name, calls, ns, 100.0 * ns / total)
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        lines.append(f"  {os.path.basename(os.path.dirname(f))}")
        for r in csv.DictReader(open(f)):
            row(r.get("Name", ""), r.get("Calls", 1), r.get("TotalDurationNs", 0), r.get("Percentage", 0))
    with open(out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.txt"))
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--passes", choices=CONTENTS)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    torch.cuda.set_device(0)
    if a.passes:
        return passes(a.passes)
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def ms(t):
        return f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"
    emit(f"components_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, {a.rounds} interleaved rounds of {a.steps} steps, median [min .. max]")
    emit("algorithmic bytes = 1 B a pixel read (the mask) + 4 B a pixel written (the root); im2col of this library: 4.3 TB/s.  mask_clean = holes + islands, "
         "min_area 100: two labellings and two apply passes.  No target was fixed for these kernels: this is what they reach.")
    first = {}
    for kind in CONTENTS:
        conn = CONN[kind]
        emit(f"{kind}, connectivity {conn}")
        for P, side in ((1, 1024), (64, 1024), (192, 1024), (192, 256)):
            m = planes(kind, P, side, dev)
            n_comp, largest, ch = check(m, conn)
            ws_cc = torch.empty((ops.L.load().vdr_connected_components_workspace_bytes(P, side, side),), dtype=torch.uint8, device=dev)
            ws_cl = torch.empty((ops.L.load().vdr_mask_clean_workspace_bytes(P, side, side),), dtype=torch.uint8, device=dev)
            r = interleaved([lambda: ops.connected_components(m, conn, workspace=ws_cc),
                             lambda: ops.mask_clean(m, 100, holes=True, islands=True, connectivity=conn, workspace=ws_cl)], a.rounds, a.steps)
            by = 5.0 * P * side * side
            first[(kind, P, side)] = r[0][0]
            emit(f"  {P:3d} x {side}^2 (plane 0: {n_comp} components, largest {largest} px, clean changed {ch}): connected_components {ms(r[0])} = "
                 f"{by / r[0][0] / 1e9:.4f} TB/s   mask_clean {ms(r[1])}")
            if side == 1024 and P in (1, 64):
                q = min(P, 8)
                t0 = time.perf_counter()
                scipy_label(m[:q], conn)
                torch.cuda.synchronize()
                t_sp = (time.perf_counter() - t0) * 1e3 * P / q
                emit(f"        scipy.ndimage.label + bincount on the host, with the device-to-host copy: {t_sp:9.3f} ms ({q} planes measured"
                     + (", scaled" if q < P else "") + f") -> the op is {t_sp / r[0][0]:.1f}x faster")
            if side == 1024 and P == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cc.label_torch(m, conn, 1, device=dev)
                torch.cuda.synchronize()
                t_lt = (time.perf_counter() - t0) * 1e3
                emit(f"        label_torch on the device (one run): {t_lt:9.3f} ms -> the op is {t_lt / r[0][0]:.1f}x faster")
            del m, ws_cc, ws_cl
    for P, side in ((64, 1024), (192, 1024)):
        base = first[("blobs", P, side)]
        for kind in ("bernoulli", "serpentine"):
            ratio = first[(kind, P, side)] / base
            emit(f"{kind} against blobs at {P} x {side}^2: {ratio:.2f}x the time" + ("  **several times slower: see the per-pass times**" if ratio > 3 else ""))
    if not a.no_end_to_end:
        from vdr import spectral
        gh = gw = 64
        rng = np.random.default_rng(5)
        parts = [(rng.random(gh * gw) < 0.59) for _ in range(16)]
        seeds = [int(np.flatnonzero(p)[0]) for p in parts]
        h = spectral._masks_and_boxes(parts, seeds, (gh, gw), dev)
        d = spectral._masks_and_boxes_device(parts, seeds, (gh, gw), dev)
        assert all(torch.equal(u, v) for u, v in zip(h, d))
        r = interleaved([lambda: spectral._masks_and_boxes(parts, seeds, (gh, gw), dev), lambda: spectral._masks_and_boxes_device(parts, seeds, (gh, gw), dev)],
                        a.rounds, a.steps)
        emit(f"the labelling step of tokencut / lost, 16 maps on a 64 x 64 grid (Bernoulli 0.59 bipartitions): host {ms(r[0])}   device {ms(r[1])}  "
             + (f"{r[0][0] / r[1][0]:.1f}x faster" if r[1][0] <= r[0][0] else f"**LOSS: {r[1][0] / r[0][0]:.2f}x slower**"))
        from segment_bench import decoder_weights
        from segment_prompt_bench import prompt_weights, sam_model
        w = decoder_weights(7)
        w.update(prompt_weights(8))
        m = sam_model(w)
        x = torch.rand((1, 3, 1024, 1024), device=dev).to(torch.bfloat16)
        kw = dict(points_per_side=16, pred_iou_thresh=-1e30, stability_score_thresh=0.0, box_nms_thresh=1.0, mask_threshold=1.0)
        k0, k1 = len(m.generate_masks(x, **kw)), len(m.generate_masks(x, min_mask_region_area=100, **kw))
        r = interleaved([lambda: m.generate_masks(x, **kw), lambda: m.generate_masks(x, min_mask_region_area=100, **kw)], max(a.rounds // 2, 3), 2)
        emit(f"generate_masks at 1024^2, 16 x 16 points (seeded weights, no filter, box_nms_thresh 1: every candidate is kept and cleaned): "
             f"without small-region removal {ms(r[0])} ({k0} masks)   with min_mask_region_area 100 {ms(r[1])} ({k1} masks): +{r[1][0] - r[0][0]:.3f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
