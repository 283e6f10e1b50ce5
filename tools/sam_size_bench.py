#!/usr/bin/env python3
"""MedSAM (SAM ViT-B image encoder) at other input sizes: slices/s at 256^2, 512^2, 768^2 and 1024^2, batch 1 and 16, in ONE
process, each next to its FLOP ratio against 1024^2 (oracle/sam_oracle.flops_per_image).  Every size loads the same native
1024^2 checkpoint (seeded weights): load_model("medsam", img_size=side).
   python tools/sam_size_bench.py [--sizes 256,512,768,1024] [--batches 1,16] [--rounds 7] [--steps 10] [--fp8 0] [--out FILE]
   python tools/sam_size_bench.py --kernel [--lib path/to/tuning/libvdr.so]
--kernel: the global-attention op alone (vdr_op_attention_relpos: table pack + rel-pos GEMM + attention kernel), interleaved
rounds.  With a tuning build (make TUNING=1) VDR_RELPOS_ANY = 1 / 2 forces the run-time-grid kernel (single / double buffered)
at any grid side, so that it can be timed against the specialised <4, 64, true> kernel at g = 64 on the same inputs; run under
`rocprofv3 --kernel-trace --stats` the per-kernel durations separate the attention kernel from the two launches before it.
--once (for profiler runs): one forward per size and batch after warm-up, no timing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
import torch  # noqa: E402

from oracle import sam_oracle as so  # noqa: E402  (weight generator and FLOP count only)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def size_bench(a, emit):
    import vdr
    sizes = [int(s) for s in a.sizes.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
    w = so.make_weights(so.SAM_VIT_B, seed=1)
    flops = {s: so.flops_per_image(so.SamCfg(img=s)) for s in sizes + [1024]}
    runs = []
    for s in sizes:
        m = vdr.load_model("medsam", weights=w, img_size=None if s == 1024 else s, fp8=a.fp8)
        for b in batches:
            x = torch.rand(b, 3, s, s).to(torch.bfloat16).cuda()
            g = s // 16
            out = torch.empty(b, g, g, 256, dtype=torch.float32, device="cuda")
            runs.append((s, b, (lambda m=m, x=x, out=out: m.engine.forward_into(x, out, vdr.OUT_ENCODER))))
    for _, _, fn in runs:  # warm every shape
        fn()
        fn()
    torch.cuda.synchronize()
    if a.once:
        for _, _, fn in runs:
            fn()
        torch.cuda.synchronize()
        return
    times = {(s, b): [] for s, b, _ in runs}
    for rnd in range(a.rounds):
        for s, b, fn in (runs if rnd & 1 else runs[::-1]):  # interleaved, alternating order
            times[(s, b)].append(timed(fn, a.steps))
    emit(f"MedSAM encoder (SAM ViT-B, 12 blocks, native 1024^2 tables) at other input sizes; fp8 = {a.fp8}; bf16 images, fp32 "
         f"neck output; {a.rounds} interleaved rounds of {a.steps} steps, median (min .. max) ms per step; kernels {vdr._lib.source_id()}")
    emit(f"{'side':>5} {'grid':>4} {'batch':>5} {'ms/step':>9} {'min':>8} {'max':>8} {'slices/s':>9} {'GFLOP/slice':>11} {'FLOP ratio':>10} "
         f"{'speed-up':>8} {'of ratio':>8}")
    for b in batches:
        base = med(times[(1024, b)]) if (1024, b) in times else None
        for s in sizes:
            t = times[(s, b)]
            ratio = flops[1024] / flops[s]
            up = base / med(t) if base else float("nan")
            emit(f"{s:>5} {s // 16:>4} {b:>5} {med(t):>9.3f} {min(t):>8.3f} {max(t):>8.3f} {b / med(t) * 1e3:>9.1f} {flops[s] / 1e9:>11.1f} "
                 f"{ratio:>10.2f} {up:>8.2f} {up / ratio:>8.2f}")


def kernel_bench(a, emit):
    from vdr import _lib as L
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    from vdr import ops
    tuning = bool(L.load().vdr_tuning_build())
    variants = [("default", "0")] + ([("any, single-buffered", "1"), ("any, double-buffered", "2")] if tuning else [])
    emit(f"vdr_op_attention_relpos (pack + rel-pos GEMM + attention), 12 heads; tuning build: {tuning}; {a.rounds} interleaved "
         f"rounds of {a.steps} calls, median (min .. max) ms per call; kernels {L.source_id()}")
    for g, B in ((64, 16), (64, 1), (48, 16), (32, 16), (32, 1), (16, 16)):
        gen = torch.Generator().manual_seed(g)
        qkv = torch.randn(B * g * g, 3 * 12 * 64, generator=gen).to(torch.bfloat16).cuda()
        rh = (torch.randn(2 * g - 1, 64, generator=gen) * 0.1).cuda()
        rw = (torch.randn(2 * g - 1, 64, generator=gen) * 0.1).cuda()
        outs, times = {}, {n: [] for n, _ in variants}

        def call(v):
            os.environ["VDR_RELPOS_ANY"] = v
            return ops.attention_relpos(qkv, rh, rw, B, g, 12)
        for n, v in variants:
            outs[n] = call(v)
        torch.cuda.synchronize()
        for rnd in range(1 if a.once else a.rounds):
            for n, v in (variants if rnd & 1 else variants[::-1]):
                times[n].append(timed(lambda: call(v), 1 if a.once else a.steps))
        ref = outs["default"].float()
        for n, _ in variants:
            t = times[n]
            d = (outs[n].float() - ref).abs().max().item()
            emit(f"g {g:>2} batch {B:>2}  {n:<22} {med(t):>8.3f} ({min(t):.3f} .. {max(t):.3f}) ms   x{med(t) / med(times['default']):.3f} of default"
                 f"   max |out - default| {d:.3e}")
    os.environ["VDR_RELPOS_ANY"] = "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,768,1024")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--fp8", type=int, default=0)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path"
    torch.cuda.set_device(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    (kernel_bench if a.kernel else size_bench)(a, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
