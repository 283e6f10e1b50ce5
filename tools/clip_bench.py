#!/usr/bin/env python3
"""CLIP / SigLIP vision towers beside the plain ViT-B/16, one process, interleaved rounds, HIP events.

    python tools/clip_bench.py [--batch 256] [--rounds 7] [--steps 5] [--warmup 3]  >  profiles/clip_bench.txt

Workloads (224^2, batch 256, bf16 images, seeded weights):
  vit_base16_224            erf-GELU                               (bench.py's model)
  clip_vit_base16_224       QuickGELU, input LayerNorm, LayerNorm fold on (default) and no_ln_fold = 1
  siglip_base16_224         tanh-GELU, no CLS token, attention-pooling head
1. ms / step and img / s of every model's token forward (VDR_OUT_TOKENS, bf16 out: all rows of all 12 blocks, the same
   work in every model) and of its feature call (CLS / get_image_features): median over the rounds, the rounds visit the
   models in turn.
2. the fc1 launch per activation: the library's profile class gemm_fc1 (HIP events around each launch), mean per launch.
3. SigLIP's pooling head at batch 256 on fixed tokens: vdr_op_attention_pool against the composition it replaces (a zero
   [B, n, 3D] buffer, k | v written into it, the full self-attention kernel, row 0 kept), and the pooling launch alone with
   its achieved GB/s (it reads B n 2D bf16 once).
One JSON line per section."""
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
    import clip_ref as cr  # (seeded weights of the towers and their heads)
    import vdr
    from oracle import vit_oracle as vo
    from vdr import ops
    torch.cuda.set_device(0)
    B = a.batch
    x = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).cuda()

    def cfg_of(name):
        c = vdr.ARCHS[name]
        return vo.VitCfg(c.img, c.patch, 3, c.dim, c.heads, c.layers, c.mlp_hidden, act=c.act, has_cls=c.has_cls, input_ln=c.input_ln,
                         ln_eps=c.ln_eps)
    models = {
        "vit_base16_224": vdr.load_model("vit_base16_224", weights=vo.make_weights(vo.CONFIGS["vit_base16_224"], seed=1)),
        "clip_vit_base16_224": vdr.load_model("clip_vit_base16_224", weights=cr.make_weights(cfg_of("clip_vit_base16_224"), "clip", 1)),
        "clip_vit_base16_224 no_ln_fold": vdr.load_model("clip_vit_base16_224", weights=cr.make_weights(cfg_of("clip_vit_base16_224"), "clip", 1),
                                                         ln_fold=False),
        "siglip_base16_224": vdr.load_model("siglip_base16_224", weights=cr.make_weights(cfg_of("siglip_base16_224"), "siglip", 1)),
    }
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds,
                      "steps_per_round": a.steps, "warmup": a.warmup}), flush=True)
    # 1. step times
    tok = interleaved({k: (lambda m=m: m.engine.forward(x, vdr.OUT_TOKENS, torch.bfloat16)) for k, m in models.items()},
                      a.rounds, a.steps, a.warmup)
    feat = interleaved({"vit_base16_224 forward_features": lambda: models["vit_base16_224"].forward_features(x),
                        "clip_vit_base16_224 forward_features": lambda: models["clip_vit_base16_224"].forward_features(x),
                        "clip_vit_base16_224 get_image_features": lambda: models["clip_vit_base16_224"].get_image_features(x),
                        "siglip_base16_224 get_image_features": lambda: models["siglip_base16_224"].get_image_features(x)},
                       a.rounds, a.steps, a.warmup)
    for sec, res in (("token forward (all rows, bf16 out)", tok), ("feature call", feat)):
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"section": sec, "workload": k, "ms_per_step_median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
                              "img_per_s": round(B / med * 1e3, 1)}), flush=True)
    # 2. fc1 per activation (profile class gemm_fc1: 12 identical launches per token forward)
    for rnd in range(3):
        for k, m in models.items():
            e = m.engine
            e.profile(True, ["gemm_fc1"])
            for _ in range(a.steps):
                e.forward(x, vdr.OUT_TOKENS, torch.bfloat16)
            torch.cuda.synchronize()
            p = e.profile_read()["gemm_fc1"]
            e.profile(False)
            print(json.dumps({"section": "fc1 launch", "round": rnd, "workload": k, "act": m.cfg.act, "launches": p["launches"],
                              "us_per_launch": round(p["ms"] / p["launches"] * 1e3, 2),
                              "tflops": round(p["flops"] / p["ms"] / 1e9, 1)}), flush=True)
    # 3. SigLIP pooling head on fixed tokens
    sm = models["siglip_base16_224"]
    head, D, H = sm.head, sm.cfg.dim, sm.cfg.heads
    tokens = sm.engine.forward(x, vdr.OUT_TOKENS, torch.bfloat16)
    n = tokens.shape[1]
    kv = ops.linear(tokens.reshape(B * n, D), head.wkv, head.bkv)

    def composition():  # the one-query attention as _CrossAttentionCls composes it from the self-attention kernel
        qkv = torch.zeros((B, n, 3 * D), dtype=torch.bfloat16, device="cuda")
        qkv[:, :, D:] = ops.linear(tokens.reshape(B * n, D), head.wkv, head.bkv).view(B, n, 2 * D)
        qkv[:, 0, :D] = head.q.to(torch.bfloat16)
        return ops.attention(qkv.view(B * n, 3 * D), B, n, H, head_dim=D // H).view(B, n, D)[:, 0, :].contiguous()

    def pooled_new():
        return ops.attention_pool(head.q, ops.linear(tokens.reshape(B * n, D), head.wkv, head.bkv), B, n, H, D // H)
    diff = (composition().float() - pooled_new().float()).abs().max().item()
    res = interleaved({"k/v GEMM + vdr_op_attention_pool": pooled_new, "k/v GEMM + zero qkv + self-attention, row 0": composition,
                       "vdr_op_attention_pool alone": lambda: ops.attention_pool(head.q, kv, B, n, H, D // H),
                       "whole head (pooled)": lambda: head.pooled(tokens)}, a.rounds, 20, a.warmup)
    nbytes = B * n * 2 * D * 2
    for k, (med, lo, hi) in res.items():
        r = {"section": "siglip pooling head", "workload": k, "ms_median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        if k.endswith("alone"):
            r.update(bytes_read=nbytes, gb_per_s=round(nbytes / med / 1e6, 1), share_of_6300=round(nbytes / med / 1e6 / 6300, 3))
        print(json.dumps(r), flush=True)
    print(json.dumps({"section": "siglip pooling head", "max_abs_diff_new_vs_composition": diff,
                      "composition_extra_alloc_bytes": B * n * 3 * D * 2}), flush=True)


if __name__ == "__main__":
    main()
