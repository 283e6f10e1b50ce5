#!/usr/bin/env python3
"""The automatic mask generator on one MI355X: what its post-processing costs next to the decode it follows.

   python tools/amg_bench.py [--rounds 9] [--steps 20] [--out profiles/amg_bench.txt] [--no-generate]

* mask_stats at 192 planes (64 points x 3 masks, tokens 1 .. 3 of [64, 4, 256, 256] read in place) and at 1 plane, 256^2 -> 1024^2,
  in algorithmic bytes / s (the 256 KB plane in, 28 bytes out) and in interpolated pixels / s, against the torch chain on the same
  device: F.interpolate, three comparisons, the sums, and _batched_mask_to_box's reductions.  Outputs are compared first.
* nms at N = 256, 1024, 4096 on heavily overlapping boxes and on all-disjoint boxes (nothing goes: the walk's longest chain).
* generate_masks end to end at 1024^2 (MedSAM ViT-B geometry, seeded weights, 32 x 32 points, 64 a batch), with the encoder, the 16
  decodes, the 16 statistics calls, the NMS, the re-decode of the kept points and the two host reads timed separately.
Interleaved medians with min and max; losses are printed as losses."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vdr  # noqa: E402
from segment_bench import decoder_weights, interleaved  # noqa: E402
from segment_prompt_bench import prompt_weights, sam_model  # noqa: E402
from vdr import amg, ops  # noqa: E402


def torch_stats(lg, size, thr, off):
    """the framework chain: the up-sampled planes are written (fp32) and read back by every reduction"""
    up = F.interpolate(lg, size=size, mode="bilinear", align_corners=False)
    counts = torch.stack([(up > thr + off).sum((-1, -2)), (up > thr).sum((-1, -2)), (up > thr - off).sum((-1, -2))], dim=-1).to(torch.int32)
    m = up > thr
    h, w = size
    in_h, in_w = torch.max(m, dim=-1)[0], torch.max(m, dim=-2)[0]
    ih, iw = torch.arange(h, device=lg.device), torch.arange(w, device=lg.device)
    bottom, top = (in_h * ih).amax(-1), (in_h * ih + h * (~in_h)).amin(-1)
    right, left = (in_w * iw).amax(-1), (in_w * iw + w * (~in_w)).amin(-1)
    empty = (right < left) | (bottom < top)
    return counts, (torch.stack([left, top, right, bottom], dim=-1) * (~empty)[..., None]).to(torch.int32)


def boxes_for(n, disjoint, dev):
    """(boxes, scores): a grid of boxes that do not touch, or seeded boxes with centres in an extent of sqrt(n) and sides of 0.5 .. 1 extent
    (about half of 256, a quarter of 1024 survive at 0.7)"""
    g = torch.Generator().manual_seed(1)
    if disjoint:
        i = torch.arange(n, dtype=torch.float32)
        x, y = (i % 64) * 4.0, (i // 64) * 4.0
        return torch.stack([x, y, x + 3.0, y + 3.0], dim=1).to(dev), torch.linspace(1.0, 0.0, n).to(dev)
    extent = n ** 0.5
    c, s = torch.rand((n, 2), generator=g) * extent, extent * (0.5 + 0.5 * torch.rand((n, 2), generator=g))
    return torch.cat([c - s / 2, c + s / 2], dim=1).to(dev), torch.rand(n, generator=g).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_bench.txt"))
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def us(t):
        return f"{t[0] * 1e3:9.1f} us [{t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}]"
    emit(f"amg_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, {a.rounds} interleaved rounds of {a.steps} steps, median [min .. max]")
    emit("mask_stats, 256^2 -> 1024^2, threshold 0, offset 1; algorithmic bytes = 256 KB in + 28 B out a plane; im2col of this library: 4.3 TB/s; "
         "the 64-problem decode these planes come from: 2.2 ms (profiles/segment_bench.txt)")
    size = (1024, 1024)
    for P, label in ((192, "192 planes (tokens 1 .. 3 of [64, 4, 256, 256], in place)"), (1, "1 plane")):
        lg4 = torch.randn((max(P // 3, 1), 4, 256, 256), device=dev) * 3
        lg = lg4[:, 1:] if P > 1 else lg4[:, 1:2]
        c0, b0 = ops.mask_stats(lg, size, 0.0, 1.0)
        c1, b1 = torch_stats(lg, size, 0.0, 1.0)
        near = int((c0 != c1).sum()) + int((b0 != b1).sum())   # (ATen's GPU kernel rounds differently: a pixel at a threshold may flip)
        r = interleaved([lambda: ops.mask_stats(lg, size, 0.0, 1.0), lambda: torch_stats(lg, size, 0.0, 1.0)], a.rounds, a.steps)
        by, px = P * (256 * 256 * 4 + 28), P * 1024 * 1024
        emit(f"  {label}: library {us(r[0])} = {by / r[0][0] / 1e9:.4f} TB/s, {px / r[0][0] / 1e6:.1f} G interpolated pixels/s   torch chain {us(r[1])}  "
             + (f"{r[1][0] / r[0][0]:.1f}x faster" if r[0][0] <= r[1][0] else f"**LOSS: {r[0][0] / r[1][0]:.2f}x slower**")
             + f"   ({near} of {c0.numel() + b0.numel()} integers differ from the torch chain's)")
    emit("nms at threshold 0.7: the matrix kernel + the one-wave walk; typical = heavily overlapping random boxes, disjoint = nothing is suppressed")
    for n in (256, 1024, 4096):
        row = []
        for disjoint in (False, True):
            b, s = boxes_for(n, disjoint, dev)
            kept, count = ops.nms(b, s, 0.7)
            r = interleaved([lambda: ops.nms(b, s, 0.7), lambda: torch.sort(s, descending=True, stable=True).indices.to(torch.int32)], a.rounds, a.steps)
            row.append(f"{'disjoint' if disjoint else 'typical '} kept {int(count):4d}: {us(r[0])} (of which the sort {r[1][0] * 1e3:.1f} us)")
        emit(f"  N {n:4d}: " + "   ".join(row))
    if not a.no_generate:
        img = 1024
        w = decoder_weights(7)
        w.update(prompt_weights(8))
        m = sam_model(w)
        x = torch.rand((1, 3, img, img), device=dev).to(torch.bfloat16)
        grid = amg.point_grid(32, img).to(dev)
        lbl = torch.ones((1, 64, 1), dtype=torch.int32, device=dev)
        emb = m.image_encoder(x)

        def decodes():
            return [m.decode_masks(emb, points=grid[s:s + 64].reshape(1, 64, 1, 2), point_labels=lbl, multimask=True) for s in range(0, 1024, 64)]
        segs = decodes()
        iou = torch.cat([s.iou[0] for s in segs]).reshape(-1)
        st = [s.stats() for s in segs]
        stab = torch.cat([v[2][0] for v in st]).reshape(-1)
        # seeded weights predict no real IoU: thresholds at quantiles of the candidates, so that a quarter survives (SAM on a photograph: a few hundred of 3072)
        t_iou, t_stab = float(iou.quantile(0.5)), float(stab[~stab.isnan()].quantile(0.5))
        kw = dict(pred_iou_thresh=t_iou, stability_score_thresh=t_stab)
        flags = (iou > t_iou) & (stab > t_stab)
        cand = flags.nonzero()[:, 0]
        boxes = torch.cat([v[1][0] for v in st]).reshape(-1, 4)[cand].float()
        one = torch.zeros(1, dtype=torch.int32, device=dev)
        emit(f"generate_masks at 1024^2, 32 x 32 points, 64 a batch, thresholds at the candidates' medians (iou {t_iou:.4f}, stability {t_stab:.4f}): "
             f"{int(cand.numel())} of 3072 pass the filter")
        r = interleaved([lambda: m.image_encoder(x), decodes, lambda: [s.stats() for s in segs], lambda: ops.nms(boxes, iou[cand], 0.7), lambda: flags.cpu(),
                         lambda: int(one.cpu())], max(a.rounds // 3, 3), 3)
        for nm, t in zip(("the encoder", "the 16 decodes of 64 points", "the 16 mask_stats calls (192 planes each)", "nms of the survivors",
                          "host read 1 (3072 flags, with its synchronise)", "host read 2 (one int32)"), r):
            emit(f"  {nm:58s} {t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]")
        # seeded weights give noise masks whose boxes span the image, so NMS at 0.7 keeps few; box_nms_thresh = 1 suppresses nothing and
        # re-decodes every survivor: the two ends of what the re-decode can cost
        for nt in (0.7, 1.0):
            ms = m.generate_masks(x, box_nms_thresh=nt, **kw)
            K, kp = len(ms), ms.points

            def redecode():
                return [m.decode_masks(emb, points=kp[s:s + 64].reshape(1, -1, 1, 2), point_labels=lbl[:, :kp[s:s + 64].shape[0]], multimask=True)
                        for s in range(0, K, 64)]
            r = interleaved([lambda: m.generate_masks(x, box_nms_thresh=nt, **kw), redecode], max(a.rounds // 3, 3), 3)
            emit(f"  box_nms_thresh {nt}: {K} kept   generate_masks end to end {r[0][0]:8.3f} ms [{r[0][1]:.3f} .. {r[0][2]:.3f}]   "
                 f"of which the re-decode of the kept points ({(K + 63) // 64} calls) {r[1][0]:8.3f} ms [{r[1][1]:.3f} .. {r[1][2]:.3f}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
