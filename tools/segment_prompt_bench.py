#!/usr/bin/env python3
"""Point / mask prompts and the volume sweep on one MI355X: what they cost next to the box decode.

   python tools/segment_prompt_bench.py [--rounds 9] [--steps 20] [--out profiles/segment_prompts_bench.txt] [--no-sweep]
                                        [--parent-lib PATH --parent-copy PATH] [--lib PATH]
   python tools/segment_prompt_bench.py --one-step      (one sweep step and nothing else: the program to put behind
                                                         `rocprofv3 --kernel-trace --stats --`, no counters in the same run)

* decode at g = 64, P = 1: vdr_mask_decode (T = 7), vdr_mask_decode_prompts with boxes only (T = 7: checked bitwise equal
  first), with a box and nine points (T = 16) and with a box and a mask prompt; interleaved medians with min and max.
  --parent-lib / --parent-copy: the parent commit's library and a second copy of it, dlopen'ed next to this one: its
  vdr_mask_decode must give this library's bits at P = 1 and P = 16, and the time difference is read against parent /
  parent-copy; then the time to build a decoder (create, set every weight, finalize), alternating between the two libraries.
  --lib: run everything on that libvdr.so instead of the package's own (the sweep of a parent build, in a process of its own).
* mask_embed alone at P = 1, 16, 64 in algorithmic TB/s (embedding 1 KB + mask 64 B in, keys 512 B out per cell) against
  the eager torch convolution chain.  decoder_keys_kernel cannot be launched alone through the ABI: its time is read from the
  kernel trace of a box-only sweep step (--one-step --no-mask-prompt).
* mask_box against its torch ops.
* a 64-slice sweep at 1024^2 (MedSAM ViT-B, seeded weights): model.propagate_masks "up" and "both" against a hand loop of
  decode_masks with a host read of the box per slice; the encoder's time is measured alone and subtracted.
Losses are printed as losses."""
import argparse
import ctypes
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
from vdr import _lib, ops  # noqa: E402
from vdr.segment import SA_EPS, MaskDecoder  # noqa: E402

MD = "prompt_encoder.mask_downscaling."


def prompt_weights(seed):
    g = torch.Generator().manual_seed(seed)
    w = {"prompt_encoder.not_a_point_embed.weight": torch.randn((1, 256), generator=g)}
    for k, shp, fan in (("0", (4, 1, 2, 2), 4), ("3", (16, 4, 2, 2), 16), ("6", (256, 16, 1, 1), 16)):
        w[MD + k + ".weight"], w[MD + k + ".bias"] = torch.randn(shp, generator=g) / fan ** 0.5, 0.1 * torch.randn(shp[0], generator=g)
    for k, d in (("1", 4), ("4", 16)):
        w[MD + k + ".weight"], w[MD + k + ".bias"] = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    return w


def pack(w):
    return torch.cat([w[MD + k].reshape(-1).float() for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias",
                                                               "6.weight", "6.bias")])


def torch_keys(emb, mask, w, eps=1e-6):
    """the eager baseline of mask_embed: the convolution chain, + emb, one rounding to bf16 -> [P * n, 256]"""
    def ln2d(x, k):
        return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w[MD + k + ".weight"], w[MD + k + ".bias"], eps).permute(0, 3, 1, 2)
    x = F.gelu(ln2d(F.conv2d(mask[:, None], w[MD + "0.weight"], w[MD + "0.bias"], stride=2), "1"))
    x = F.gelu(ln2d(F.conv2d(x, w[MD + "3.weight"], w[MD + "3.bias"], stride=2), "4"))
    x = F.conv2d(x, w[MD + "6.weight"], w[MD + "6.bias"])
    return (x + emb).permute(0, 2, 3, 1).reshape(-1, 256).to(torch.bfloat16)


def torch_mask_box(lg, prev, img, margin):
    P, H, W = lg.shape
    on = lg > 0
    xs, ys = on.any(dim=1), on.any(dim=2)
    ix, iy = torch.arange(W, device=lg.device), torch.arange(H, device=lg.device)
    x0, x1 = torch.where(xs, ix, 1 << 30).amin(1).float(), (torch.where(xs, ix, -1).amax(1) + 1).float()
    y0, y1 = torch.where(ys, iy, 1 << 30).amin(1).float(), (torch.where(ys, iy, -1).amax(1) + 1).float()
    sx, sy = float(img) / W, float(img) / H
    box = torch.stack([x0 * sx - margin, y0 * sy - margin, x1 * sx + margin, y1 * sy + margin], 1).clamp(0.0, float(img))
    area = on.reshape(P, -1).sum(1).to(torch.int32)
    return torch.where((area > 0)[:, None], box, prev), area


def foreign_decoder(path, w, g, img, mlp_dim=2048, problems=1):
    """a box-prompt decoder handle on the library at `path` (one built before the prompt entry points existed lacks them);
    decode(emb [1, 256, g, g], boxes [problems, 4], lg, iou), .close()"""
    lib = _lib.bind(ctypes.CDLL(path), skip_missing=True)
    cfg = _lib.vdr_mask_decoder_config(grid=g, img=img, channels=256, heads=8, depth=2, mlp_dim=mlp_dim, attention_downsample_rate=2, mask_tokens=4,
                                       upscale_channels_1=64, upscale_channels_2=32, iou_head_depth=3, **SA_EPS)
    h = ctypes.c_void_p()
    assert lib.vdr_mask_decoder_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    for i in range(lib.vdr_mask_decoder_num_weights(h)):
        name = lib.vdr_mask_decoder_weight_name(h, i).decode()
        t = w[name].detach().float().contiguous()
        assert lib.vdr_mask_decoder_set_weight(h, name.encode(), t.data_ptr(), (ctypes.c_int64 * t.dim())(*t.shape), t.dim()) == 0
    assert lib.vdr_mask_decoder_finalize(h) == 0
    n = ctypes.c_size_t()
    assert lib.vdr_mask_decoder_workspace_bytes(h, problems, ctypes.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")

    def decode(emb, boxes, lg, iou):
        assert lib.vdr_mask_decode(h, emb.data_ptr(), 0, boxes.data_ptr(), 1, problems, ws.data_ptr(), ws.numel(), lg.data_ptr(), iou.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream) == 0
    decode.close = lambda: lib.vdr_mask_decoder_destroy(h)
    return decode


def sam_model(w):
    from oracle import sam_oracle as so  # (weight generator only)
    ew = dict(so.make_weights(so.SAM_VIT_B, seed=1))
    ew.update(w)
    return vdr.load_model("medsam", weights=ew)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_prompts_bench.txt"))
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-copy")
    ap.add_argument("--lib")
    ap.add_argument("--one-step", action="store_true")
    ap.add_argument("--no-mask-prompt", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)  # before the first load()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    w = decoder_weights(7)
    w.update(prompt_weights(8))
    g, img = 64, 1024
    if a.one_step:   # two slices of a sweep on a decoder alone (no encoder in the trace): seed decode + mask_box, one step
        dec = MaskDecoder(w, g, img, dev, **SA_EPS)
        emb = torch.randn((2, 256, g, g), device=dev)
        box = torch.tensor([[[200.0, 220.0, 800.0, 790.0]]], device=dev)
        for _ in range(3):   # (the last repetition is the one to read; the first warms up)
            lg, _ = dec.decode(emb[:1], box)
            nxt, _ = ops.mask_box(lg[:, 0, 0], box[0], img, margin=8.0)
            dec.decode(emb[1:], nxt[None], mask_input=None if a.no_mask_prompt else lg[:, :, 0])
        torch.cuda.synchronize()
        print("one sweep step done")
        return
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(t):
        return f"{t[0]:7.3f} [{t[1]:.3f} .. {t[2]:.3f}]"
    emit(f"segment_prompt_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, library {os.path.relpath(_lib.LIB_PATH, ROOT)}, "
         f"{a.rounds} interleaved rounds of {a.steps} steps, median ms [min .. max]")
    dec = MaskDecoder(w, g, img, dev, **SA_EPS)
    emb = torch.randn((1, 256, g, g), device=dev)
    boxes = torch.tensor([[[200.0, 220.0, 800.0, 790.0]]], device=dev)
    pts = (torch.rand((1, 1, 9, 2), generator=torch.Generator().manual_seed(1)) * img).to(dev)
    lbl = torch.tensor([[[1, 0, 1, 1, 0, 1, 0, 0, 1]]], dtype=torch.int32, device=dev)
    lg0, iou0 = dec.decode(emb, boxes)
    mask = lg0[:, :, 0].contiguous()
    pr = _lib.vdr_mask_prompts(boxes=boxes.data_ptr())
    ws = torch.empty(dec.workspace_bytes(1, 7), dtype=torch.uint8, device=dev)
    lg1, iou1 = torch.empty_like(lg0), torch.empty_like(iou0)

    def new_entry():
        _lib.check(dec.lib.vdr_mask_decode_prompts(dec.h, emb.data_ptr(), 0, ctypes.byref(pr), 1, 1, ws.data_ptr(), ws.numel(), lg1.data_ptr(),
                                                   iou1.data_ptr(), torch.cuda.current_stream().cuda_stream))
    new_entry()
    torch.cuda.synchronize()
    same = torch.equal(lg0, lg1) and torch.equal(iou0, iou1)
    emit(f"decode at g 64, P 1 (outputs checked first: boxes only through vdr_mask_decode_prompts bitwise equal to vdr_mask_decode: {same})")
    assert same
    fns = [lambda: dec.decode(emb, boxes), new_entry, lambda: dec.decode(emb, boxes, pts, lbl), lambda: dec.decode(emb, boxes, mask_input=mask)]
    names = ["vdr_mask_decode, T 7 (the yardstick)", "vdr_mask_decode_prompts, boxes only, T 7", "a box and nine points, T 16", "a box and a mask prompt, T 7"]
    res = interleaved(fns, a.rounds, a.steps)
    for nm, t in zip(names, res):
        d = t[0] - res[0][0]
        emit(f"  {nm:44s} {fmt(t)}  {d:+.3f} ms against the yardstick" + ("" if d <= max(res[0][2] - res[0][1], 0.0) or nm.startswith("vdr_mask_decode,")
                                                                          else "  **outside the yardstick's own min .. max**"))
    if a.parent_lib:
        import time
        this = os.path.abspath(_lib.LIB_PATH)
        for P in (1, 16):   # vdr_mask_decode on the three libraries, raw ctypes calls with preallocated outputs on each
            bx = (boxes[0] + torch.arange(P, device=dev)[:, None] * torch.tensor([3.0, 2.0, -2.0, -3.0], device=dev)).contiguous()
            decs = [foreign_decoder(p, w, g, img, problems=P) for p in (a.parent_lib, a.parent_copy or a.parent_lib, this)]
            outs = [(torch.empty((1, P, 4, 4 * g, 4 * g), device=dev), torch.empty((1, P, 4), device=dev)) for _ in decs]
            for dc, (lg, iou) in zip(decs, outs):
                dc(emb, bx, lg, iou)
            torch.cuda.synchronize()
            same = all(torch.equal(lg, outs[2][0]) and torch.equal(iou, outs[2][1]) for lg, iou in outs[:2])
            emit(f"the parent's library on the same weights, P {P}: vdr_mask_decode bitwise equal to this library's: {same}")
            assert same
            r = interleaved([lambda dc=dc, o=o: dc(emb, bx, *o) for dc, o in zip(decs, outs)], a.rounds, a.steps)
            spread = abs(r[0][0] - r[1][0])
            emit(f"  parent {fmt(r[0])}  parent copy {fmt(r[1])}  (difference of two parents {spread:.4f} ms)  this library {fmt(r[2])}")
            d = r[2][0] - r[0][0]
            emit(f"  this - parent = {d:+.4f} ms: " + ("inside" if d <= max(spread, r[0][2] - r[0][1]) else "**SLOWER, OUTSIDE**") + " the parents' spread / min .. max")
            for dc in decs:
                dc.close()
        ms = {p: [] for p in (a.parent_lib, this)}   # load time: create, set every weight, finalize (g 64: the float64 tables dominate)
        for _ in range(5):
            for p in ms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dc = foreign_decoder(p, w, g, img)
                torch.cuda.synchronize()
                ms[p].append((time.perf_counter() - t0) * 1e3)
                dc.close()
        emit("building a decoder at g 64, mlp_dim 2048 (create, set every weight, finalize): 5 per library, alternating, wall clock (ms)")
        for p, v in ms.items():
            emit(f"  {os.path.relpath(p, ROOT):40s} median {sorted(v)[2]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   " + " ".join(f"{x:.1f}" for x in v))
        d = sorted(ms[this])[2] - sorted(ms[a.parent_lib])[2]
        rng = max(ms[a.parent_lib]) - min(ms[a.parent_lib])
        emit(f"  median this - parent = {d:+.1f} ms; range of the parent {rng:.1f} ms -> " + ("not slower beyond the parent's range" if d <= rng else "**SLOWER**"))
    emit("mask_embed alone at g 64, algorithmic bytes (embedding 1 KB + mask 64 B in, keys 512 B out per cell) / time; im2col of this library: 4.3 TB/s")
    packed = pack(w).to(dev)
    wd = {k: v.to(dev) for k, v in w.items() if k.startswith(MD)}
    for P in (1, 16, 64):
        e = torch.randn((P, 256, g, g), device=dev)
        cl = e.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        m = torch.randn((P, 4 * g, 4 * g), device=dev) * 3
        out = torch.empty((P * g * g, 256), dtype=torch.bfloat16, device=dev)
        got, ref = ops.mask_embed(e, m, packed, out=out).float(), torch_keys(e, m, wd).float()
        rel = float((got - ref).norm() / ref.norm())
        assert rel < 1e-2 and torch.equal(ops.mask_embed(cl, m, packed), out)
        r = interleaved([lambda: ops.mask_embed(e, m, packed, out=out), lambda: ops.mask_embed(cl, m, packed, out=out), lambda: torch_keys(e, m, wd)],
                        a.rounds, a.steps)
        by = P * g * g * (1024 + 64 + 512)
        emit(f"  P {P:2d}: channel-first {r[0][0] * 1e3:8.1f} us [{r[0][1] * 1e3:.1f} .. {r[0][2] * 1e3:.1f}] = {by / r[0][0] / 1e9:.3f} TB/s   channel-last "
             f"{r[1][0] * 1e3:8.1f} us [{r[1][1] * 1e3:.1f} .. {r[1][2] * 1e3:.1f}] = {by / r[1][0] / 1e9:.3f} TB/s   torch eager {r[2][0] * 1e3:8.1f} us "
             f"({r[2][0] / r[0][0]:.1f}x)  relL2 to torch {rel:.1e}" + ("  **misses the im2col's 4.3 TB/s**" if by / min(r[0][0], r[1][0]) / 1e9 < 4.3 else ""))
    emit("mask_box on token 0 of [P, 4, 256, 256] against its torch ops (outputs checked bitwise first)")
    for P in (1, 2, 16):
        lg = torch.randn((P, 4, 256, 256), device=dev)
        prev = torch.zeros((P, 4), device=dev)
        b0, a0 = ops.mask_box(lg[:, 0], prev, img, margin=8.0)
        b1, a1 = torch_mask_box(lg[:, 0], prev, img, 8.0)
        assert torch.equal(b0, b1) and torch.equal(a0, a1)
        r = interleaved([lambda: ops.mask_box(lg[:, 0], prev, img, margin=8.0), lambda: torch_mask_box(lg[:, 0], prev, img, 8.0)], a.rounds, a.steps)
        emit(f"  P {P:2d}: library {r[0][0] * 1e3:7.1f} us [{r[0][1] * 1e3:.1f} .. {r[0][2] * 1e3:.1f}]  torch {r[1][0] * 1e3:7.1f} us  "
             + (f"{r[1][0] / r[0][0]:.1f}x faster" if r[0][0] <= r[1][0] else f"**LOSS: {r[0][0] / r[1][0]:.2f}x slower**"))
    if not a.no_sweep:
        Z = a.slices
        emit(f"a {Z}-slice sweep at 1024^2 (MedSAM ViT-B, seeded weights), from slice 0 (up) or slice {Z // 2} (both); encoder in chunks of 16")
        m = sam_model(w)
        x = torch.rand((Z, 3, img, img), device=dev).to(torch.bfloat16)
        box = torch.tensor([200.0, 220.0, 800.0, 790.0])

        def encoder():
            return torch.cat([m.image_encoder(x[s:s + 16]) for s in range(0, Z, 16)])

        def hand(use_mask):
            e = encoder()
            b, prev = box.reshape(1, 1, 4), None
            for z in range(Z):
                seg = m.decode_masks(e[z:z + 1], b, mask_input=prev if use_mask else None)
                lg = seg.low_res_logits[:, 0, 0]
                nb_, _ = torch_mask_box(lg, b.reshape(1, 4).to(dev).float(), img, 8.0)
                b = torch.tensor(nb_.tolist()).reshape(1, 1, 4)       # the host read per slice
                prev = lg[:, None]
        fns = [encoder, lambda: m.propagate_masks(x, box, 0, direction="up"), lambda: m.propagate_masks(x, box, Z // 2, direction="both"),
               lambda: m.propagate_masks(x, box, 0, direction="up", use_mask_prompt=False), lambda: hand(True), lambda: hand(False)]
        r = interleaved(fns, max(a.rounds // 3, 3), 1)
        enc = r[0][0]
        emit(f"  encoder alone {fmt(r[0])} ms")
        for nm, t in zip(("propagate_masks up, mask prompt", "propagate_masks both (two-problem steps), mask prompt", "propagate_masks up, box only",
                          "hand loop (host read per slice), mask prompt", "hand loop, box only"), r[1:]):
            emit(f"  {nm:56s} {fmt(t)} ms   sweep alone {(t[0] - enc):8.3f} ms = {(t[0] - enc) / Z:.3f} ms / slice")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
