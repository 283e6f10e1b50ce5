#!/usr/bin/env python3
"""Box prompt -> mask on one MI355X: what the mask decoder costs, alone and on top of the encoder.

   python tools/segment_bench.py [--rounds 9] [--steps 20] [--out profiles/segment_bench.txt] [--no-e2e]

* decode alone at g = 64 for (B, nb) = (1, 1), (16, 1), (1, 64) and at g = 32 for (16, 1): the library's decode
  (vdr/segment.py MaskDecoder.decode) against a plain bf16 torch module of the same definition (this file's own copy: tools
  do not import tests) on the same device and inputs, medians of interleaved rounds with the spread; launches per decode of
  both (the library's count is MaskDecoder.LAUNCHES plus its torch set-up ops; both are counted with torch.profiler).
* end to end at 1024^2: model.segment against model.image_encoder alone at B = 1 and 16 (seeded MedSAM ViT-B weights).
* the two memory-bound kernels in algorithmic bytes per second: cross attention (k and v read once), the upscale tail
  (its rows read once, the logits written once).
Losses are printed as losses."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vdr  # noqa: E402
from vdr import ops  # noqa: E402
from vdr.segment import SA_EPS, MaskDecoder, fourier_pe  # noqa: E402

C = 256


def decoder_weights(seed, mlp_dim=2048):
    """seeded decoder weights under segment_anything's names (timing only: N(0, 1) / sqrt(fan_in) linears)"""
    g = torch.Generator().manual_seed(seed)
    w = {}

    def lin(p, o, i, s=1.0):
        w[p + ".weight"], w[p + ".bias"] = torch.randn((o, i), generator=g) * s / math.sqrt(i), torch.randn(o, generator=g) * 0.1

    def ln(p, d=C):
        w[p + ".weight"], w[p + ".bias"] = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)

    def attn(p, inner):
        for n in ("q_proj", "k_proj", "v_proj"):
            lin(p + n, inner, C, 2.0)
        lin(p + "out_proj", C, inner)
    w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"] = torch.randn((2, 128), generator=g)
    w["prompt_encoder.no_mask_embed.weight"] = torch.randn((1, C), generator=g)
    for i in range(4):
        w[f"prompt_encoder.point_embeddings.{i}.weight"] = torch.randn((1, C), generator=g)
    w["mask_decoder.iou_token.weight"], w["mask_decoder.mask_tokens.weight"] = torch.randn((1, C), generator=g), torch.randn((4, C), generator=g)
    for i in range(2):
        p = f"mask_decoder.transformer.layers.{i}."
        attn(p + "self_attn.", C)
        attn(p + "cross_attn_token_to_image.", 128)
        attn(p + "cross_attn_image_to_token.", 128)
        lin(p + "mlp.lin1", mlp_dim, C)
        lin(p + "mlp.lin2", C, mlp_dim)
        for j in range(1, 5):
            ln(p + f"norm{j}")
    attn("mask_decoder.transformer.final_attn_token_to_image.", 128)
    ln("mask_decoder.transformer.norm_final_attn")
    U = "mask_decoder.output_upscaling."
    w[U + "0.weight"], w[U + "0.bias"] = torch.randn((C, 64, 2, 2), generator=g) / 16, torch.randn(64, generator=g) * 0.1
    ln(U + "1", 64)
    w[U + "3.weight"], w[U + "3.bias"] = torch.randn((64, 32, 2, 2), generator=g) / 8, torch.randn(32, generator=g) * 0.1
    for m in range(4):
        for j, (o, i_) in enumerate(((C, C), (C, C), (32, C))):
            lin(f"mask_decoder.output_hypernetworks_mlps.{m}.layers.{j}", o, i_)
    for j, (o, i_) in enumerate(((C, C), (C, C), (4, C))):
        lin(f"mask_decoder.iou_prediction_head.layers.{j}", o, i_)
    return w


class TorchDecoder:
    """the same definition as a plain bf16 torch module (eager): the baseline"""

    def __init__(self, w, g, img, dev, eps):
        self.w = {k: v.to(dev).to(torch.bfloat16) for k, v in w.items()}
        self.g, self.img, self.eps = g, img, eps
        gauss = w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"].double()
        t = (torch.arange(g, dtype=torch.float64) + 0.5) / g
        yy, xx = torch.meshgrid(t, t, indexing="ij")
        self.kpe = fourier_pe(torch.stack([xx, yy], -1), gauss).reshape(g * g, C).to(dev).to(torch.bfloat16)
        self.gauss = gauss.to(dev)

    def lin(self, x, p):
        return F.linear(x, self.w[p + ".weight"], self.w[p + ".bias"])

    def ln(self, x, p, eps):
        return F.layer_norm(x, (x.shape[-1],), self.w[p + ".weight"], self.w[p + ".bias"], eps)

    def attend(self, q, k, v, p):
        q, k, v = self.lin(q, p + "q_proj"), self.lin(k, p + "k_proj"), self.lin(v, p + "v_proj")
        P, D = q.shape[0], q.shape[-1]
        q, k, v = (t.reshape(P, -1, 8, D // 8).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // 8), dim=-1) @ v
        return self.lin(a.transpose(1, 2).reshape(P, -1, D), p + "out_proj")

    def decode(self, emb, boxes):
        w, g = self.w, self.g
        B, nb = boxes.shape[:2]
        P, n = B * nb, g * g
        c = (boxes.to(emb.device).double().reshape(-1, 2, 2) + 0.5) / float(self.img)
        sp = fourier_pe(c, self.gauss).to(torch.bfloat16)
        sp = sp + torch.stack([w["prompt_encoder.point_embeddings.2.weight"][0], w["prompt_encoder.point_embeddings.3.weight"][0]])
        tok = torch.cat([torch.cat([w["mask_decoder.iou_token.weight"], w["mask_decoder.mask_tokens.weight"]])[None].expand(P, -1, -1), sp], 1)
        pe = tok
        keys = (emb.to(torch.bfloat16).reshape(B, C, n).transpose(1, 2) + w["prompt_encoder.no_mask_embed.weight"]).repeat_interleave(nb, 0)
        kpe = self.kpe
        T = "mask_decoder.transformer."
        for i in range(2):
            p = T + f"layers.{i}."
            if i == 0:
                tok = self.attend(tok, tok, tok, p + "self_attn.")
            else:
                tok = tok + self.attend(tok + pe, tok + pe, tok, p + "self_attn.")
            tok = self.ln(tok, p + "norm1", self.eps["ln_eps"])
            tok = self.ln(tok + self.attend(tok + pe, keys + kpe, keys, p + "cross_attn_token_to_image."), p + "norm2", self.eps["ln_eps"])
            tok = self.ln(tok + self.lin(torch.relu(self.lin(tok, p + "mlp.lin1")), p + "mlp.lin2"), p + "norm3", self.eps["ln_eps"])
            keys = self.ln(keys + self.attend(keys + kpe, tok + pe, tok, p + "cross_attn_image_to_token."), p + "norm4", self.eps["ln_eps"])
        tok = self.ln(tok + self.attend(tok + pe, keys + kpe, keys, T + "final_attn_token_to_image."), T + "norm_final_attn", self.eps["final_ln_eps"])
        U = "mask_decoder.output_upscaling."
        x = keys.transpose(1, 2).reshape(P, C, g, g)
        x = F.conv_transpose2d(x, w[U + "0.weight"], w[U + "0.bias"], stride=2)
        x = F.gelu(self.ln(x.permute(0, 2, 3, 1), U + "1", self.eps["ln2d_eps"]).permute(0, 3, 1, 2))
        x = F.gelu(F.conv_transpose2d(x, w[U + "3.weight"], w[U + "3.bias"], stride=2))
        hy = []
        for m in range(4):
            p = f"mask_decoder.output_hypernetworks_mlps.{m}.layers."
            hy.append(self.lin(torch.relu(self.lin(torch.relu(self.lin(tok[:, 1 + m], p + "0")), p + "1")), p + "2"))
        hy = torch.stack(hy, 1)
        lg = (hy @ x.reshape(P, 32, 16 * n)).reshape(B, nb, 4, 4 * g, 4 * g)
        p = "mask_decoder.iou_prediction_head.layers."
        iou = self.lin(torch.relu(self.lin(torch.relu(self.lin(tok[:, 0], p + "0")), p + "1")), p + "2")
        return lg.float(), iou.float().reshape(B, nb, 4)


def timed(fn, steps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def interleaved(fns, rounds, steps):
    """medians (and min, max) of `rounds` interleaved rounds, round 0 a warm-up, the order alternating"""
    t = [[] for _ in fns]
    for r in range(rounds + 1):
        for i in (range(len(fns)) if r & 1 else reversed(range(len(fns)))):
            v = timed(fns[i], steps)
            if r:
                t[i].append(v)
    return [(sorted(v)[len(v) // 2], min(v), max(v)) for v in t]


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # (a profiler that cannot attach is no reason to lose the timings)
        return f"n/a ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.txt"))
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)
    emit(f"segment_bench: {torch.cuda.get_device_name(0)}, kernels {vdr.source_id()}, {a.rounds} interleaved rounds of {a.steps} steps, "
         "median ms [min .. max]")
    w = decoder_weights(7)
    emit("decode alone (embedding in, 4 low-res logit maps + IoU out), real geometry: 256 ch, 8 heads, depth 2, mlp_dim 2048")
    for g, B, nb in ((64, 1, 1), (64, 16, 1), (64, 1, 64), (32, 16, 1)):
        dec = MaskDecoder(w, g, 16 * g, dev, **SA_EPS)
        ref = TorchDecoder(w, g, 16 * g, dev, SA_EPS)
        emb = torch.randn((B, C, g, g), device=dev)
        boxes = torch.tensor([[[100.0, 120.0, 16.0 * g - 100, 16.0 * g - 90]]]).expand(B, nb, 4).contiguous()
        fl, ft = (lambda: dec.decode(emb, boxes)), (lambda: ref.decode(emb, boxes))
        (lm, l0, l1), (tm, t0, t1) = interleaved([fl, ft], a.rounds, a.steps)
        lg, _ = fl()
        rg, _ = ft()
        rel = float((lg - rg).norm() / rg.norm())
        verdict = f"{tm / lm:.2f}x faster" if lm <= tm else f"**LOSS: {lm / tm:.2f}x slower**"
        emit(f"  g {g:2d} B {B:2d} nb {nb:2d}: library {lm:7.3f} [{l0:.3f} .. {l1:.3f}]  torch bf16 {tm:7.3f} [{t0:.3f} .. {t1:.3f}]  {verdict}"
             f"  launches: library {launches(fl)} (of which {MaskDecoder.LAUNCHES} the library's own), torch {launches(ft)}"
             f"  (relL2 between the two {rel:.2e})")
    emit("the memory-bound kernels, algorithmic bytes / time")
    for P, tk in ((16, 4096), (64, 4096)):
        kv = torch.randn((P * tk, 384), device=dev).to(torch.bfloat16)
        q = torch.randn((P * 7, 128), device=dev).to(torch.bfloat16)
        tab = torch.randn((tk, 128), device=dev)
        ms = interleaved([lambda: ops.cross_attention(q, kv[:, :128], kv[:, 128:256], P, 7, tk, 8, 16, k_add=tab)], a.rounds, a.steps)[0]
        by = P * tk * 256 * 2
        emit(f"  cross_attention 7 x {tk}, dh 16, P {P}: {ms[0] * 1e3:8.1f} us [{ms[1] * 1e3:.1f} .. {ms[2] * 1e3:.1f}]  k + v {by / 1e6:.1f} MB once -> "
             f"{by / ms[0] / 1e9:.3f} TB/s (im2col of this library: 4.3 TB/s)")
    for P in (1, 16, 64):
        g = 64
        x = torch.randn((P * g * g * 4, 64), device=dev).to(torch.bfloat16)
        W2, b2, hy = torch.randn((128, 64), device=dev).to(torch.bfloat16), torch.randn(32, device=dev), torch.randn((P, 4, 32), device=dev)
        out = torch.empty((P, 4, 4 * g, 4 * g), device=dev)
        ms = interleaved([lambda: ops.mask_upscale(x, W2, b2, hy, P, g, out=out)], a.rounds, a.steps)[0]
        by = x.numel() * 2 + out.numel() * 4
        emit(f"  mask_upscale g 64, P {P}: {ms[0] * 1e3:8.1f} us [{ms[1] * 1e3:.1f} .. {ms[2] * 1e3:.1f}]  rows in + logits out {by / 1e6:.1f} MB -> "
             f"{by / ms[0] / 1e9:.3f} TB/s")
    if not a.no_e2e:
        from oracle import sam_oracle as so  # (weight generator only)
        emit("end to end at 1024^2 (MedSAM ViT-B, seeded weights): segment = image_encoder + decode, one box per image")
        ew = dict(so.make_weights(so.SAM_VIT_B, seed=1))
        ew.update(w)
        m = vdr.load_model("medsam", weights=ew)
        for B in (1, 16):
            x = torch.rand((B, 3, 1024, 1024), device=dev).to(torch.bfloat16)
            boxes = torch.tensor([[[200.0, 220.0, 800.0, 790.0]]]).expand(B, 1, 4).contiguous()
            (em, e0, e1), (sm, s0, s1) = interleaved([lambda: m.image_encoder(x), lambda: m.segment(x, boxes)], a.rounds, max(a.steps // 4, 3))
            emit(f"  B {B:2d}: image_encoder {em:8.3f} [{e0:.3f} .. {e1:.3f}]  segment {sm:8.3f} [{s0:.3f} .. {s1:.3f}]  the decoder adds "
                 f"{sm - em:+.3f} ms = {100 * (sm - em) / em:+.1f} %")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
