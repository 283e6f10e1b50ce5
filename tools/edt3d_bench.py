#!/usr/bin/env python3
"""Exact 3-D Euclidean distance transforms of mask volumes with voxel spacing on one MI355X: what the op costs, by content.

   python tools/edt3d_bench.py [--rounds 5] [--steps 3] [--out profiles/edt3d_bench.txt] [--no-end-to-end]
   python tools/edt3d_bench.py --passes blobs|bernoulli|corner|full_outside     (a few calls only: the run rocprofv3 traces)
   python tools/edt3d_bench.py --kernel-stats DIR --out FILE                     (appends the per-kernel times of traced runs)

* vdr.ops.distance_transform_3d at 64 x 512^2, 128 x 256^2 and 300 x 512^2, spacing (2560, 717, 717) (2.5 x 0.7 x 0.7 mm in units of
  2^-10 mm): d2 alone, the thresholded volume only at a 3 mm radius (the early exits), and d2 with the peak, on (a) blobs,
  (b) a Bernoulli(0.5) volume, and two adversaries of the outward searches: (c) all set but ONE clear corner voxel (every search
  runs to the far face), (d) all set with every axis outside.  Every rung is checked first: the smallest against scipy, every one
  against closed forms or the thresholded volume against d2.
* yardsticks: scipy.ndimage.distance_transform_edt(sampling=) on the host INCLUDING the device-to-host copy of the mask; the 2-D op
  (vdr.ops.distance_transform) run over the same bytes as Z planes, which is what the third pass and the weights cost;
  algorithmic bytes / s beside the 2-D op's.
* algorithmic bytes: the mask read once (1 byte a voxel), the output written once (8 bytes a voxel for d2, 1 for the thresholded
  volume); the 2-D op writes 4 bytes a pixel.
* end to end: VolumeSegmentation.compare with and without a spacing; a propagate_masks sweep started from inner_voxel.
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
SHAPES = ((64, 512, 512), (128, 256, 256), (300, 512, 512))
Q = (2560, 717, 717)
R2 = 9 * 2**20            # 3 mm: floor(3^2 / 2^-20)
NONE = 2**63 - 1


def volume(kind, shape, dev):
    Z, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(3)
    if kind == "blobs":
        low = torch.randn((1, 1, max(Z // 8, 2), H // 32, W // 32), generator=g) * 3
        return (F.interpolate(low.to(dev), size=shape, mode="trilinear", align_corners=False)[0, 0] > 1.0).to(torch.uint8)
    if kind == "bernoulli":
        return (torch.rand(shape, generator=g) < 0.5).to(torch.uint8).to(dev)
    m = torch.ones(shape, dtype=torch.uint8, device=dev)
    if kind == "corner":
        m[0, 0, 0] = 0
    return m


def scipy_d2(mask_np, outside=False):
    from scipy import ndimage
    sel = np.pad(mask_np != 0, 1) if outside else mask_np != 0
    d = ndimage.distance_transform_edt(sel, sampling=[float(v) for v in Q])
    d2 = np.rint(d * d).astype(np.int64)
    return d2[1:-1, 1:-1, 1:-1] if outside else d2


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


def check(kind, m, against_scipy):
    outside = kind == "full_outside"
    d2, peak = ops.distance_transform_3d(m, Q, 1, outside, return_peak=True)
    within = ops.distance_transform_3d(m, Q, 1, outside, threshold=R2)
    assert torch.equal(within, (d2 <= R2).to(torch.uint8)), kind            # the early exits change no bit
    Z, H, W = m.shape
    zz = torch.arange(Z, device=m.device)[:, None, None]
    yy = torch.arange(H, device=m.device)[None, :, None]
    xx = torch.arange(W, device=m.device)[None, None, :]
    if kind == "corner":
        assert torch.equal(d2, (Q[0] * zz) ** 2 + (Q[1] * yy) ** 2 + (Q[2] * xx) ** 2), kind
    if kind == "full_outside":
        want = torch.minimum(torch.minimum(Q[0] * torch.minimum(zz + 1, Z - zz), Q[1] * torch.minimum(yy + 1, H - yy)), Q[2] * torch.minimum(xx + 1, W - xx)) ** 2
        assert torch.equal(d2, want.expand(Z, H, W)), kind
    if against_scipy:
        assert np.array_equal(d2.cpu().numpy(), scipy_d2(m.cpu().numpy(), outside)), kind
    top = int(d2.max())
    assert int(peak[0, 0]) == top and (top == 0 or int(d2.reshape(-1)[int(peak[0, 1])]) == top)
    return top


def passes(kind):
    dev = torch.device("cuda", 0)
    m = volume(kind, SHAPES[0], dev)
    for _ in range(3):
        ops.distance_transform_3d(m, Q, 1, kind == "full_outside", return_peak=True)
        ops.distance_transform_3d(m, Q, 1, kind == "full_outside", threshold=R2)
    torch.cuda.synchronize()


def kernel_stats(directory, out):
    """the edt3_* rows of every traced --passes run under `directory` (rocprofv3's csv or rocpd database), appended to `out`"""
    import csv
    import re
    import sqlite3
    lines = [f"per-pass times from rocprofv3 --kernel-trace --stats (a run of its own per content: {SHAPES[0]}, 3 calls with d2 and peak and 3 thresholded only)"]
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
            short = re.search(r"(edt3_\w+_kernel)", name)
            if short:
                lines.append(f"    {short.group(1):18s} calls {int(calls):4d}  total {ns / 1e6:9.3f} ms  average {ns / calls / 1e3:9.1f} us  "
                             f"{100.0 * ns / total:5.1f} % of the run's kernel time")
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        lines.append(f"  {os.path.relpath(os.path.dirname(f), directory).split(os.sep)[0]}")
        for r in csv.DictReader(open(f)):
            short = re.search(r"(edt3_\w+_kernel)", r.get("Name", ""))
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt3d_bench.txt"))
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
    emit(f"edt3d_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, {a.rounds} interleaved rounds of {a.steps} steps, median [min .. max]")
    emit(f"spacing {Q} (2.5 x 0.7 x 0.7 mm / 2^-10), threshold r2 = {R2} (3 mm).  algorithmic bytes = 1 B a voxel read + the output written once "
         "(8 B d2, 1 B thresholded; the 2-D op: 4 B d2).  No target was fixed for these kernels: this is what they reach.")
    first = {}
    for kind in CONTENTS:
        outside = kind == "full_outside"
        emit(f"{kind}" + (" (every axis outside)" if outside else ""))
        for shape in SHAPES:
            m = volume(kind, shape, dev)
            Z, H, W = shape
            top = check(kind, m, against_scipy=shape == SHAPES[1])
            ws = torch.empty((ops.L.load().vdr_distance_transform_3d_workspace_bytes(1, Z, H, W),), dtype=torch.uint8, device=dev)
            ws2 = torch.empty((ops.L.load().vdr_distance_transform_workspace_bytes(Z, H, W),), dtype=torch.uint8, device=dev)
            fns = [lambda: ops.distance_transform_3d(m, Q, 1, outside, workspace=ws),
                   lambda: ops.distance_transform_3d(m, Q, 1, outside, threshold=R2, workspace=ws),
                   lambda: ops.distance_transform_3d(m, Q, 1, outside, return_peak=True, workspace=ws),
                   lambda: ops.distance_transform(m, 1, outside, workspace=ws2)]
            r = interleaved(fns, a.rounds, a.steps)
            n = float(Z * H * W)
            first[(kind, shape)] = r[0][0]

            def rate(t, by):
                return f"{by * n / t[0] / 1e9:.4f} TB/s"
            emit(f"  {Z} x {H} x {W} (largest d2 {top if top < NONE else 'NONE'}): d2 {ms(r[0])} = {rate(r[0], 9)}")
            emit(f"        thresholded only (3 mm) {ms(r[1])} = {rate(r[1], 2)}  -> {r[0][0] / r[1][0]:.2f}x the speed of d2"
                 + ("  **the early exit does not show here**" if r[1][0] > 0.8 * r[0][0] else ""))
            emit(f"        d2 + peak {ms(r[2])}")
            emit(f"        the 2-D op slice by slice on the same bytes {ms(r[3])} = {rate(r[3], 5)}  -> 3-D is {r[0][0] / r[3][0]:.2f}x its time"
                 + ("  **LOSS against 2x**" if r[0][0] > 2 * r[3][0] else ""))
            if shape in SHAPES[:2]:
                t_sp = host_timed(lambda: scipy_d2(m.cpu().numpy(), outside), max(a.rounds // 2, 2))
                emit(f"        scipy.ndimage.distance_transform_edt(sampling=) on the host, with the device-to-host copy: {ms(t_sp)} -> the op is "
                     f"{t_sp[0] / r[0][0]:.0f}x faster")
            del m, ws, ws2
    for shape in SHAPES:
        base = first[("blobs", shape)]
        for kind in ("bernoulli", "corner", "full_outside"):
            ratio = first[(kind, shape)] / base
            emit(f"{kind} against blobs at {shape}: {ratio:.2f}x the time" + ("  **several times slower: the searches' worst case**" if ratio > 3 else ""))
    if not a.no_end_to_end:
        from segment_bench import decoder_weights
        from segment_prompt_bench import prompt_weights, sam_model
        w = decoder_weights(7)
        w.update(prompt_weights(8))
        m = sam_model(w)
        Z = 64
        x = torch.rand((Z, 3, 1024, 1024), device=dev).to(torch.bfloat16)
        box = torch.tensor([300.0, 280.0, 700.0, 760.0])
        va, vb = m.propagate_masks(x, box, Z // 2), m.propagate_masks(x, box, Z // 2, point_prompt="inner")
        rounds = max(a.rounds // 2, 3)
        sp = (2.5, 0.7, 0.7)
        got = va.compare(vb, size=(512, 512), spacing=sp)
        t_2d, t_3d = host_timed(lambda: va.compare(vb, size=(512, 512)), rounds), host_timed(lambda: va.compare(vb, size=(512, 512), spacing=sp), rounds)
        emit(f"VolumeSegmentation.compare, {Z} slices at 512^2: slice by slice {ms(t_2d)} ({Z} results)   with spacing {sp} {ms(t_3d)} (one result, "
             f"hd {float(got['hd'][0]):.3f} mm)" + (f"  **LOSS: {t_3d[0] / t_2d[0]:.2f}x the time**" if t_3d[0] > t_2d[0] else f"  {t_2d[0] / t_3d[0]:.1f}x faster"))
        masks = va.masks((512, 512))

        def sweep_from_inner_voxel():
            zyx, lab = mo.inner_voxel(masks, sp)
            z = int(zyx[0, 0]) if int(lab[0]) == 1 else Z // 2               # one synchronisation: the slice to start from
            return m.propagate_masks(x, box, z)
        t_mid, t_in = host_timed(lambda: m.propagate_masks(x, box, Z // 2), rounds), host_timed(sweep_from_inner_voxel, rounds)
        t_iv = interleaved([lambda: mo.inner_voxel(masks, sp)], rounds, 3)[0]
        emit(f"propagate_masks over {Z} slices of 1024^2 (seeded weights): from the middle slice {ms(t_mid)}   started from inner_voxel {ms(t_in)} "
             f"(inner_voxel alone {ms(t_iv)}): {t_in[0] - t_mid[0]:+.3f} ms" + ("  **LOSS**" if t_in[0] > t_mid[0] else ""))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
