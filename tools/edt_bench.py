#!/usr/bin/env python3
"""Exact Euclidean distance transforms of mask planes on one MI355X: what the op costs, by content.

   python tools/edt_bench.py [--rounds 5] [--steps 5] [--out profiles/edt_bench.txt] [--no-end-to-end]
   python tools/edt_bench.py --passes blobs|bernoulli|corner|full_outside     (a few calls only: the run rocprofv3 traces)
   python tools/edt_bench.py --kernel-stats DIR --out FILE                     (appends the per-kernel times of traced runs)

* vdr.ops.distance_transform at 1, 64 and 192 planes of 1024^2 and 192 planes of 256^2: d2 alone, d2 with nearest, and the
  thresholded plane only (r2 = 25), on (a) SAM-like blobs, (b) Bernoulli(0.5) planes, and two adversaries of the outward search:
  (c) all set but ONE clear pixel in a corner (every search runs to the plane's edge), (d) all set with outside = 1.
  Every shape is checked against scipy first (plane 0; closed forms for the adversaries).
* yardsticks: scipy.ndimage.distance_transform_edt on the host INCLUDING the device-to-host copy of the masks (measured on at
  most 4 planes and scaled: it is linear in the planes), vdr.morphology.edt_torch on the device (one 256^2 plane: its column
  step is an H x H x W tensor), and vdr.morphology.dilate(r = 5) against scipy's binary_dilation with the disc.
* algorithmic bytes / s: the mask read once (1 byte a pixel), the output written once (4 bytes a pixel for d2, 8 with nearest,
  1 for the thresholded plane).
* end to end: a 64-slice propagate_masks sweep with and without point_prompt="inner"; VolumeSegmentation.compare on the device
  against the host route (masks copied to the host, scipy's transforms).
Every figure, the yardsticks included, is a median of interleaved rounds after a warm-up round (segment_bench.interleaved; the
host routes are timed on the host clock the same way); losses are printed as losses."""
import argparse
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
from vdr import morphology as mo, ops  # noqa: E402

CONTENTS = ("blobs", "bernoulli", "corner", "full_outside")
NONE = 2**31 - 1


def planes(kind, P, side, dev):
    g = torch.Generator(device="cpu").manual_seed(3)
    if kind == "blobs":
        low = torch.randn((P, 1, side // 16, side // 16), generator=g) * 3
        return (F.interpolate(low.to(dev), size=(side, side), mode="bilinear", align_corners=False)[:, 0] > 1.0).to(torch.uint8)
    if kind == "bernoulli":
        return (torch.rand((P, side, side), generator=g) < 0.5).to(torch.uint8).to(dev)   # seeded on the host: the same planes every run
    m = torch.ones((P, side, side), dtype=torch.uint8, device=dev)
    if kind == "corner":
        m[:, 0, 0] = 0
    return m


def scipy_d2(mask_np, outside=False):
    from scipy import ndimage
    sel = np.pad(mask_np != 0, 1) if outside else mask_np != 0
    d = ndimage.distance_transform_edt(sel)
    d2 = np.rint(d * d).astype(np.int64)
    return d2[1:-1, 1:-1] if outside else d2


def host_timed(fn, rounds):
    """(median, min, max) ms of `rounds` runs of a host route after one warm-up run (it synchronises by its own copies)"""
    fn()
    v = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return sorted(v)[len(v) // 2], min(v), max(v)


def check(kind, mask):
    outside = kind == "full_outside"
    d2 = ops.distance_transform(mask, outside=outside)
    within = ops.distance_transform(mask, outside=outside, threshold=25)
    assert torch.equal(within, (d2 <= 25).to(torch.uint8))
    want = scipy_d2(mask[0].cpu().numpy(), outside)
    assert np.array_equal(d2[0].cpu().numpy(), want), kind
    if not outside:
        d2n, nearest = ops.distance_transform(mask, return_nearest=True)
        assert torch.equal(d2n, d2)
        sel = mask[0] != 0
        if bool((~sel).any()):
            W = mask.shape[2]
            ny, nx = torch.div(nearest[0][sel], W, rounding_mode="floor"), nearest[0][sel] % W
            yy, xx = torch.nonzero(sel, as_tuple=True)
            assert torch.equal((yy - ny) ** 2 + (xx - nx) ** 2, d2[0][sel].long()) and not bool(sel[ny, nx].any())
    return int(d2[0].max())


def passes(kind):
    dev = torch.device("cuda", 0)
    m = planes(kind, 64, 1024, dev)
    for _ in range(5):
        ops.distance_transform(m, outside=kind == "full_outside", return_peak=True)
    torch.cuda.synchronize()


def kernel_stats(directory, out):
    """the edt_* rows of every traced --passes run under `directory` (rocprofv3's rocpd database), appended to `out`"""
    import re
    import sqlite3
    lines = ["per-pass times from rocprofv3 --kernel-trace --stats (a run of its own per content: 64 planes of 1024^2, 5 calls with d2 and peak)"]
    for f in sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)):
        lines.append(f"  {os.path.relpath(os.path.dirname(f), directory).split(os.sep)[0]}")
        con = sqlite3.connect(f)
        tables = [r[0] for r in con.execute("select name from sqlite_master where type in ('table', 'view')")]
        t = "kernels" if "kernels" in tables else next((n for n in tables if n.startswith("kernels")), None)
        if t is None:
            lines.append(f"    no kernel table in {os.path.basename(f)}")
            continue
        rows = con.execute(f"select name, count(*), sum(end - start) from {t} group by name order by 3 desc").fetchall()
        total = sum(r[2] for r in rows)
        for name, calls, ns in rows:
            short = re.search(r"(edt_\w+_kernel)", name)
            if short:
                lines.append(f"    {short.group(1):18s} calls {int(calls):4d}  total {ns / 1e6:9.3f} ms  average {ns / calls / 1e3:9.1f} us  "
                             f"{100.0 * ns / total:5.1f} % of the run's kernel time")
    import csv
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        lines.append(f"  {os.path.relpath(os.path.dirname(f), directory).split(os.sep)[0]}")
        for r in csv.DictReader(open(f)):
            short = re.search(r"(edt_\w+_kernel)", r.get("Name", ""))
            if short:
                calls, ns = int(r.get("Calls", 1)), float(r.get("TotalDurationNs", 0))
                lines.append(f"    {short.group(1):18s} calls {calls:4d}  total {ns / 1e6:9.3f} ms  average {ns / calls / 1e3:9.1f} us  "
                             f"{float(r.get('Percentage', 0)):5.1f} % of the run's kernel time")
    with open(out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_bench.txt"))
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
    emit(f"edt_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, {a.rounds} interleaved rounds of {a.steps} steps, median [min .. max]")
    emit("algorithmic bytes = 1 B a pixel read (the mask) + the output written once (4 B d2, 8 B d2 + nearest, 1 B thresholded); im2col of this "
         "library: 4.3 TB/s.  No target was fixed for these kernels: this is what they reach.")
    first = {}
    for kind in CONTENTS:
        outside = kind == "full_outside"
        emit(f"{kind}" + (" (outside = 1; nearest is not defined there)" if outside else ""))
        for P, side in ((1, 1024), (64, 1024), (192, 1024), (192, 256)):
            m = planes(kind, P, side, dev)
            top = check(kind, m)
            ws = torch.empty((ops.L.load().vdr_distance_transform_workspace_bytes(P, side, side),), dtype=torch.uint8, device=dev)
            fns = [lambda: ops.distance_transform(m, outside=outside, workspace=ws), lambda: ops.distance_transform(m, outside=outside, threshold=25, workspace=ws)]
            if not outside:
                fns.append(lambda: ops.distance_transform(m, return_nearest=True, workspace=ws))
            r = interleaved(fns, a.rounds, a.steps)
            px = float(P * side * side)
            first[(kind, P, side)] = r[0][0]

            def rate(t, by):
                v = by * px / t[0] / 1e9
                return f"{v:.4f} TB/s" + ("  **below the im2col's 4.3 TB/s**" if v < 4.3 else "")
            emit(f"  {P:3d} x {side}^2 (plane 0: largest d2 {top if top < NONE else 'NONE'}): d2 {ms(r[0])} = {rate(r[0], 5)}")
            emit(f"        thresholded only {ms(r[1])} = {rate(r[1], 2)}" + (f"   d2 + nearest {ms(r[2])} = {rate(r[2], 9)}" if not outside else ""))
            if side == 1024 and P in (1, 64):
                q = min(P, 4)

                def host_edt():
                    host = m[:q].cpu().numpy()
                    for p in range(q):
                        scipy_d2(host[p], outside)
                t_sp = tuple(v * P / q for v in host_timed(host_edt, a.rounds))
                emit(f"        scipy.ndimage.distance_transform_edt on the host, with the device-to-host copy: {ms(t_sp)} ({q} planes measured"
                     + (", scaled" if q < P else "") + f") -> the op is {t_sp[0] / r[0][0]:.1f}x faster")
            if side == 1024 and P == 1 and kind in ("blobs", "bernoulli"):
                from scipy import ndimage
                yy, xx = np.mgrid[-5:6, -5:6]
                disc = yy * yy + xx * xx <= 25
                want = ndimage.binary_dilation(m[0].cpu().numpy() != 0, disc)
                assert np.array_equal(mo.dilate(m, 5)[0].cpu().numpy() != 0, want)
                rd = interleaved([lambda: mo.dilate(m, 5)], a.rounds, a.steps)
                t_sp = host_timed(lambda: ndimage.binary_dilation(m[0].cpu().numpy() != 0, disc), a.rounds)
                emit(f"        dilate(r = 5) {ms(rd[0])}; scipy's binary_dilation with the disc, with the copy: {ms(t_sp)} -> {t_sp[0] / rd[0][0]:.1f}x faster")
            if side == 256 and kind in ("blobs", "corner"):
                one = m[:1]
                assert torch.equal(mo.edt_torch(one, outside=outside, device=dev), ops.distance_transform(one, outside=outside))
                r1 = interleaved([lambda: mo.edt_torch(one, outside=outside, device=dev), lambda: ops.distance_transform(one, outside=outside)], a.rounds, a.steps)
                emit(f"        edt_torch on the device, ONE 256^2 plane: {ms(r1[0])}; the op on that plane {ms(r1[1])} -> {r1[0][0] / r1[1][0]:.1f}x faster")
            del m, ws
    for P, side in ((64, 1024), (192, 1024), (192, 256)):
        base = first[("blobs", P, side)]
        for kind in ("bernoulli", "corner", "full_outside"):
            ratio = first[(kind, P, side)] / base
            emit(f"{kind} against blobs at {P} x {side}^2: {ratio:.2f}x the time" + ("  **several times slower: the search's worst case**" if ratio > 3 else ""))
    if not a.no_end_to_end:
        from segment_bench import decoder_weights
        from segment_prompt_bench import prompt_weights, sam_model
        w = decoder_weights(7)
        w.update(prompt_weights(8))
        m = sam_model(w)
        Z = 64
        x = torch.rand((Z, 3, 1024, 1024), device=dev).to(torch.bfloat16)
        box = torch.tensor([300.0, 280.0, 700.0, 760.0])
        r = interleaved([lambda: m.propagate_masks(x, box, Z // 2), lambda: m.propagate_masks(x, box, Z // 2, point_prompt="inner")], max(a.rounds // 2, 3), 1)
        d = (r[1][0] - r[0][0]) / Z
        emit(f"propagate_masks over {Z} slices of 1024^2 (seeded weights): without the click {ms(r[0])}   with point_prompt='inner' {ms(r[1])}: "
             f"{d * 1e3:+.1f} us a slice" + ("  **LOSS**" if d > 0 else ""))
        va, vb = m.propagate_masks(x, box, Z // 2), m.propagate_masks(x, box, Z // 2, point_prompt="inner")

        def host_route():
            from scipy import ndimage
            a_, b_ = va.masks().cpu().numpy(), vb.masks().cpu().numpy()
            cross = ndimage.generate_binary_structure(2, 1)
            out = []
            for p in range(Z):
                sa, sb = a_[p] ^ ndimage.binary_erosion(a_[p], cross), b_[p] ^ ndimage.binary_erosion(b_[p], cross)
                if sa.any() and sb.any():
                    ab, ba = ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]
                    out.append((max(ab.max(), ba.max()), np.percentile(np.concatenate([ab, ba]), 95), (ab.mean() + ba.mean()) / 2))
            return out
        got, want = va.compare(vb), host_route()
        rounds = max(a.rounds // 2, 3)
        t_d, t_h = host_timed(lambda: va.compare(vb), rounds), host_timed(host_route, rounds)
        t_dev, t_host = t_d[0], t_h[0]
        print(f"compare: hd of slice {Z // 2} {float(got['hd'][Z // 2]):.3f}, {len(want)} slices with both surfaces on the host route")
        emit(f"VolumeSegmentation.compare, {Z} slices at 1024^2: on the device {ms(t_d)}   host route (copy, scipy) {ms(t_h)}  "
             + (f"{t_host / t_dev:.1f}x faster" if t_dev <= t_host else f"**LOSS: {t_dev / t_host:.2f}x slower**"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
