#!/usr/bin/env python3
"""Cost of guided upsampling of dense descriptors: vdr_op_upsample_guided against the same quantity from torch ops on the same
inputs -- a loop over the (2r+1)^2 window offsets that accumulates weight times gathered features in fp32 -- and against its
algorithmic bytes; model.upsample_descriptors on a 64 x 64 box against the alternative it replaces, set_patch_stride(4) +
extract_descriptors cropped to the same region.

    python tools/upsample_bench.py [--rounds R] [--e2e 0|1] > profiles/upsample_bench.txt

One process, one device; the sides alternate round by round (who goes first alternates too), device events around `steps`
calls after a warm-up; medians over the rounds.  Every shape is checked against the torch loop before it is timed (worst
difference relative to the largest entry printed; above 2e-2 -- two bf16 roundings -- the tool stops).
JSON lines:
  kernel "upsample_guided": workload, images, grid, patch, stride, C, radius, box, items (workgroups: images x cells x chunks x
      channel groups), tile_rows_filled (the share of the 128 staged pixel rows that are real), vdr_ms, torch_ms,
      torch_over_vdr, algo_mb (the output written once plus the reached descriptors and the guide under them read once),
      tb_per_s (algo bytes / time; the overlapping im2col of this project reaches 4.3 TB/s), worst_rel.
  the end-to-end line: upsample_descriptors on a 64 x 64 box against stride-4 descriptors cropped to that region, ms per call:
      the cost of the alternative, not a parity check (the two are different quantities)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

IM2COL_TBS = 4.3
R, SIG_S, SIG_R = 2, 1.0, 0.1
#            name                                              B   H     p   s   C      features       box
WORKLOADS = (("vit_base16 224^2 keys, 8 images, whole image",  8,  224,  16, 16, 768,   torch.bfloat16, None),
             ("vit_base16 224^2 stride 8, 8 images, whole",    8,  224,  16, 8,  768,   torch.bfloat16, None),
             ("vit_base16 224^2 keys, 64 images, 64x64 box",   64, 224,  16, 16, 768,   torch.bfloat16, (83, 67, 147, 131)),
             ("medsam neck 1024^2, 1 image, 128x128 box",      1,  1024, 16, 16, 256,   torch.float32,  (411, 523, 539, 651)),
             ("binned keys (13056 ch), 8 images, 32x32 box",   8,  224,  16, 16, 13056, torch.bfloat16, (101, 90, 133, 122)))


def span_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, rounds, budget_ms=150.0):
    """median ms per call of each fn over `rounds` alternating rounds; steps per round sized from a first timed call"""
    first = []
    for f in fns:
        f()
        first.append(span_ms(f, 1))
    steps = [max(1, min(200, int(budget_ms / max(t, 1e-3)))) for t in first]
    times = [[] for _ in fns]
    for r in range(rounds):
        order = range(len(fns)) if r & 1 else reversed(range(len(fns)))
        for i in order:
            times[i].append(span_ms(fns[i], steps[i]))
    return [sorted(t)[len(t) // 2] for t in times]


def torch_guided(F, G, p, s, r, cs, cr, box, out_dtype):
    """the same quantity from torch ops: F [B, gh, gw, C], G [B, Cg, H, W] -> [B, hb, wb, C]"""
    from vdr import upsample
    B, gh, gw, C = F.shape
    H, W = G.shape[2:]
    y0, x0, y1, x1 = box
    dev = F.device
    glr = torch.nn.functional.avg_pool2d(G.float(), p, stride=s)
    i0 = upsample.nearest_patch(H, p, s)[y0:y1].to(dev)
    j0 = upsample.nearest_patch(W, p, s)[x0:x1].to(dev)
    Y = torch.arange(y0, y1, device=dev)
    X = torch.arange(x0, x1, device=dev)
    Gb = G[:, :, y0:y1, x0:x1].float()
    acc = torch.zeros((B, y1 - y0, x1 - x0, C), dtype=torch.float32, device=dev)
    Z = torch.zeros((B, y1 - y0, x1 - x0), dtype=torch.float32, device=dev)
    for a in range(-r, r + 1):
        i = i0 + a
        iok, ic = (i >= 0) & (i < gh), i.clamp(0, gh - 1)
        dy = (2 * Y + 1 - p - 2 * s * i).float() * 0.5
        for b in range(-r, r + 1):
            j = j0 + b
            jok, jc = (j >= 0) & (j < gw), j.clamp(0, gw - 1)
            dx = (2 * X + 1 - p - 2 * s * j).float() * 0.5
            d = Gb - glr[:, :, ic][:, :, :, jc]
            t = -(dy[:, None] ** 2 + dx[None, :] ** 2) * cs - (d * d).sum(1) * cr
            w = torch.where((iok[:, None] & jok[None, :]) & (t >= -64.0), torch.exp(t), torch.zeros_like(t))
            acc += w.unsqueeze(-1) * F[:, ic][:, :, jc].float()
            Z += w
    near = F[:, i0][:, :, j0].float()
    return torch.where((Z > 0).unsqueeze(-1), acc / Z.clamp_min(1e-38).unsqueeze(-1), near).to(out_dtype)


def bench_ops(rounds):
    from vdr import ops, upsample
    gen = torch.Generator(device="cuda").manual_seed(3)
    for name, B, H, p, s, C, fdt, box in WORKLOADS:
        g = (H - p) // s + 1
        F = torch.randn((B, g, g, C), generator=gen, device="cuda").to(fdt)
        # a piecewise-smooth guide: blobs on a ramp, so that the range term has edges to follow
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device="cuda"), torch.linspace(0, 1, H, device="cuda"), indexing="ij")
        G = torch.stack([((yy * (3 + c) + xx * (2 + b)) % 1.0 > 0.5).float() * 0.6 + 0.2 * xx for b in range(B) for c in range(3)])
        G = G.reshape(B, 3, H, H).contiguous()
        bx = box if box is not None else (0, 0, H, H)
        cs, cr = ops.upsample_coefficients(s, SIG_S, SIG_R)
        odt = fdt
        run = lambda: ops.upsample_guided(F, G, p, s, radius=R, sigma_spatial=SIG_S, sigma_range=SIG_R, box=box, out_dtype=odt)  # noqa: E731
        ref = lambda: torch_guided(F, G, p, s, R, cs, cr, bx, odt)  # noqa: E731
        got, want = run().float(), ref().float()
        rel = float((got - want).abs().max() / want.abs().max())
        del got, want
        near_y, near_x = upsample.nearest_patch(H, p, s)[bx[0]:bx[2]], upsample.nearest_patch(H, p, s)[bx[1]:bx[3]]
        cells = (int(near_y.max()) - int(near_y.min()) + 1) * (int(near_x.max()) - int(near_x.min()) + 1)
        per_cell = max(int(torch.bincount(near_y).max()) * int(torch.bincount(near_x).max()), 1)
        chunks = -(-per_cell // 128)
        groups = -(-((C + 127) // 128) // 8)
        npix = (bx[2] - bx[0]) * (bx[3] - bx[1])
        pi = (max(int(near_y.min()) - R, 0), min(int(near_y.max()) + R, g - 1))
        pj = (max(int(near_x.min()) - R, 0), min(int(near_x.max()) + R, g - 1))
        reached = (pi[1] - pi[0] + 1) * (pj[1] - pj[0] + 1)
        foot = ((pi[1] - pi[0]) * s + p) * ((pj[1] - pj[0]) * s + p)
        algo = B * (npix * C * F.element_size() + reached * C * F.element_size() + foot * 3 * 4)
        line = {"kernel": "upsample_guided", "workload": name, "images": B, "grid": [g, g], "patch": p, "stride": s, "C": C,
                "radius": R, "box": list(bx), "features": str(fdt).split(".")[-1], "items": B * cells * chunks * groups,
                "tile_rows_filled": round(npix / (128.0 * cells * chunks), 3), "worst_rel": float(f"{rel:.3e}")}
        if not rel <= 2e-2:
            print(json.dumps(dict(line, error="differs from the torch loop")), flush=True)
            sys.exit(1)
        ms = interleaved([run, ref], rounds)
        line.update(vdr_ms=round(ms[0], 4), torch_ms=round(ms[1], 4), torch_over_vdr=round(ms[1] / ms[0], 2),
                    algo_mb=round(algo / 1e6, 2), tb_per_s=round(algo / (ms[0] * 1e9), 3), im2col_tb_per_s=IM2COL_TBS)
        print(json.dumps(line), flush=True)
        del F, G


def bench_e2e(rounds):
    import vdr
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    B, box = 8, (83, 67, 147, 131)
    x = torch.rand(B, 3, 224, 224).to(torch.bfloat16).cuda()

    def up():
        return model.upsample_descriptors(x, facet="key", box=box)

    def fine():
        model.set_patch_stride(4)
        d = model.extract_descriptors(x, facet="key", reshape=True)  # [B, 53, 53, D]: one descriptor per 4 pixels
        model.set_patch_stride(16)
        return d[:, (box[0] - 6) // 4:(box[2] - 6) // 4, (box[1] - 6) // 4:(box[3] - 6) // 4]

    ms = interleaved([up, fine], rounds, budget_ms=100.0)
    model.set_patch_stride(16)
    fwd = interleaved([lambda: model.extract_descriptors(x, facet="key", reshape=True)], rounds, budget_ms=100.0)
    print(json.dumps({"workload": "vit_base16 224^2 keys, 64x64 box: upsample_descriptors vs set_patch_stride(4) + crop", "images": B,
                      "box": list(box), "upsample_descriptors_ms": round(ms[0], 3), "stride16_extract_alone_ms": round(fwd[0], 3),
                      "stride4_extract_crop_ms": round(ms[1], 3), "stride4_over_upsample": round(ms[1] / ms[0], 2),
                      "note": "pixel-resolution 64x64 descriptors against 16x16 stride-4 descriptors of the same region"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e", type=int, default=1)
    args = ap.parse_args()
    import vdr
    torch.cuda.set_device(0)
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds}), flush=True)
    bench_ops(args.rounds)
    if args.e2e:
        bench_e2e(args.rounds)


if __name__ == "__main__":
    main()
