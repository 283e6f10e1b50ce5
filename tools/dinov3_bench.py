#!/usr/bin/env python3
"""DINOv3 / DINOv2-with-registers beside the plain ViT-B/16, one process, interleaved rounds, HIP events.

    python tools/dinov3_bench.py [--batch 256] [--rounds 7] [--steps 5] [--warmup 3]  >  profiles/dinov3_bench.txt

Workloads (batch 256, bf16 images, seeded weights):
  vit_base16_224                 bench.py's model, 197 tokens
  dinov3_vitb16                  4 registers, LayerScale, 2-D RoPE: 201 tokens
  dinov3_vitb16 rope=0           the same handle geometry without the rotation: what the RoPE pass costs a forward
  dinov3_vitb16 448^2            set_input_size(448, 448): 789 tokens (its own group: another image batch)
  dinov2_base14_reg_518 224^2    set_input_size(224, 224): 261 tokens, pos_embed resampled
1. ms / step and img / s of every model's token forward (VDR_OUT_TOKENS, bf16 out) and CLS feature call: median over the
   rounds, the rounds visit the models in turn.
2. the RoPE launch alone (vdr_op_rope2d on a [batch * 201, 3 * 768] activation, 5 prefix rows) with its achieved GB/s: it
   reads and writes q and k of the patch rows once (the tables stay in cache), and the same inside the forward from the
   profile class it is booked under (assemble: the prefix-row launch + 12 rotations).
One JSON line per entry."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, rounds, steps, warmup):
    """{name: fn} -> {name: (median, min, max) ms per call}; every round times each fn once, in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, steps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import dinov3_ref as dr  # (seeded weights with register tokens)
    import vdr
    from oracle import vit_oracle as vo
    from vdr import ops
    torch.cuda.set_device(0)
    B = a.batch

    def images(side, seed):
        return torch.rand(B, 3, side, side, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()

    def build(arch, **override):
        c = vdr.VdrConfig(**{**vdr.ARCHS[arch].__dict__, **override})
        vit = vo.VitCfg(c.img, c.patch, 3, c.dim, c.heads, c.layers, c.mlp_hidden, act=c.act, layerscale=c.layerscale, has_pos=c.has_pos,
                        ln_eps=c.ln_eps)
        return vdr.VitDescriptorModel(c, dr.make_weights(dr.RegCfg(vit, c.n_register, c.rope, c.rope_theta), seed=1), arch)

    x224, x448 = images(224, 0), images(448, 1)
    models = {
        "vit_base16_224": (vdr.load_model("vit_base16_224", weights=vo.make_weights(vo.CONFIGS["vit_base16_224"], seed=1)), x224),
        "dinov3_vitb16": (build("dinov3_vitb16"), x224),
        "dinov3_vitb16 rope=0": (build("dinov3_vitb16", rope=False), x224),
        "dinov2_base14_reg_518 224^2": (build("dinov2_base14_reg_518").set_input_size(224, 224), x224),
        "dinov3_vitb16 448^2": (build("dinov3_vitb16").set_input_size(448, 448), x448),
    }
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds,
                      "steps_per_round": a.steps, "warmup": a.warmup}), flush=True)
    tok = interleaved({k: (lambda m=m, x=x: m.engine.forward(x, vdr.OUT_TOKENS, torch.bfloat16)) for k, (m, x) in models.items()},
                      a.rounds, a.steps, a.warmup)
    feat = interleaved({k + " forward_features": (lambda m=m, x=x: m.forward_features(x)) for k, (m, x) in models.items()},
                       a.rounds, a.steps, a.warmup)
    for sec, res in (("token forward (all rows, bf16 out)", tok), ("feature call (CLS)", feat)):
        for k, (med, lo, hi) in res.items():
            m = models[k.replace(" forward_features", "")][0]
            print(json.dumps({"section": sec, "workload": k, "tokens": m.engine.n_tokens, "ms_per_step_median": round(med, 4),
                              "min": round(lo, 4), "max": round(hi, 4), "img_per_s": round(B / med * 1e3, 1)}), flush=True)
    d = tok["dinov3_vitb16"][0] - tok["dinov3_vitb16 rope=0"][0]
    print(json.dumps({"section": "token forward (all rows, bf16 out)", "dinov3_vitb16 minus rope=0 (ms, medians)": round(d, 4),
                      "per_block_us": round(d / 12 * 1e3, 2)}), flush=True)
    # 2. the RoPE launch
    m3 = models["dinov3_vitb16"][0]
    c = m3.cfg
    H, dh, P, N = c.heads, c.dim // c.heads, c.n_prefix, m3.engine.n_tokens
    qkv = torch.randn(B * N, 3 * c.dim, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    cos, sin = ops.rope2d_table(m3.grid, dh, c.rope_theta, device="cuda")
    res = interleaved({"vdr_op_rope2d alone": lambda: ops.rope2d(qkv, B, N, P, H, dh, cos, sin)}, a.rounds, 20, a.warmup)
    nbytes = B * (N - P) * 2 * c.dim * 2 * 2  # q and k of the patch rows, bf16, read and written
    for k, (med, lo, hi) in res.items():
        print(json.dumps({"section": "rope launch", "workload": k, "rows": B * (N - P), "us_median": round(med * 1e3, 2),
                          "min": round(lo * 1e3, 2), "max": round(hi * 1e3, 2), "bytes_moved": nbytes,
                          "gb_per_s": round(nbytes / med / 1e6, 1)}), flush=True)
    for rnd in range(3):
        for k in ("dinov3_vitb16", "dinov3_vitb16 rope=0"):
            e = models[k][0].engine
            e.profile(True, ["assemble"])
            for _ in range(a.steps):
                e.forward(x224, vdr.OUT_TOKENS, torch.bfloat16)
            torch.cuda.synchronize()
            p = e.profile_read()["assemble"]
            e.profile(False)
            print(json.dumps({"section": "assemble class inside the forward", "round": rnd, "workload": k, "launches": p["launches"],
                              "ms_per_forward": round(p["ms"] / a.steps, 4)}), flush=True)


if __name__ == "__main__":
    main()
