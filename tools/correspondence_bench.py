#!/usr/bin/env python3
"""Cost of the dense correspondences: vdr_op_nn_cosine (row norms, the fused tile kernel and the fold of the partial maxima:
all three launches) against the same result composed from torch ops on the same bf16 inputs -- normalize, bmm, max over
both dims, which materialises the [pairs, t, t] similarity matrix -- and find_correspondences end to end beside two
extract_descriptors calls.

    python tools/correspondence_bench.py [--rounds R] [--e2e 0|1] > profiles/correspondence_bench.txt

One process, one device; the two sides alternate round by round (who goes first alternates too), device events around
`steps` calls after a warm-up; medians over the rounds.  JSON lines:
  kernel "nn_cosine": workload, pairs, t, d, ms (kernel) and torch_ms, torch_over_kernel, the kernel's
      2 * t * t * d * pairs FLOP over its time as TF/s and as a share of the 2.5 PF dense bf16 peak, the MB of similarity
      matrix (fp32) that is never written, and whether the two agree (arg-maxima equal where torch's bf16 matrix has no tie
      at its maximum; the values within bf16 rounding of the torch side).
  workload lines: find_correspondences(x1, x2) against extract_descriptors(x1) + extract_descriptors(x2) (same facet, bin,
      hierarchy) on one ViT-B/16 handle, ms per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

PEAK_BF16 = 2.5e15

WORKLOADS = (("vit_base16 224^2 stride 16, unbinned", 64, 196, 768),
             ("vit_base16 224^2 stride 16, binned h=2", 64, 196, 13056),
             ("vit_base16 224^2 stride 8, binned h=2", 32, 729, 13056),
             ("vit_base16 512^2 stride 8, binned h=2", 1, 3969, 13056),
             ("vit_base16 512^2 stride 8, binned h=2", 8, 3969, 13056))


def torch_nn(x, y):
    xn, yn = torch.nn.functional.normalize(x, dim=-1), torch.nn.functional.normalize(y, dim=-1)
    s = torch.bmm(xn, yn.transpose(1, 2))
    r, c = s.max(dim=2), s.max(dim=1)
    return r.values, r.indices, c.values, c.indices


def span_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, rounds, budget_ms=250.0):
    """median ms per call of each fn over `rounds` alternating rounds; steps per round sized from a first timed call"""
    first = []
    for f in fns:
        f()
        first.append(span_ms(f, 1))
    steps = [max(1, min(50, int(budget_ms / max(t, 1e-3)))) for t in first]
    times = [[] for _ in fns]
    for r in range(rounds):
        order = range(len(fns)) if r & 1 else reversed(range(len(fns)))
        for i in order:
            times[i].append(span_ms(fns[i], steps[i]))
    return [sorted(t)[len(t) // 2] for t in times], [min(t) for t in times], steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e", type=int, default=1)
    args = ap.parse_args()
    import vdr
    from vdr import _lib as L
    torch.cuda.set_device(0)
    lib = L.load()
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds}), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    for name, P, t, d in WORKLOADS:
        gen = torch.Generator(device="cuda").manual_seed(t + d)
        x = torch.randn(P, t, d, device="cuda", generator=gen).to(torch.bfloat16)
        y = torch.randn(P, t, d, device="cuda", generator=gen).to(torch.bfloat16)
        work = torch.empty(lib.vdr_nn_cosine_work_bytes(P, t, t), dtype=torch.uint8, device="cuda")
        rs, cs = torch.empty(P, t, device="cuda"), torch.empty(P, t, device="cuda")
        ri, ci = torch.empty(P, t, dtype=torch.int32, device="cuda"), torch.empty(P, t, dtype=torch.int32, device="cuda")

        def run():
            L.check(lib.vdr_op_nn_cosine(x.data_ptr(), d, t * d, t, y.data_ptr(), d, t * d, t, P, d, work.data_ptr(), rs.data_ptr(),
                                         ri.data_ptr(), cs.data_ptr(), ci.data_ptr(), stream))

        (ms, tms), (ms_min, tms_min), steps = interleaved([run, lambda: torch_nn(x, y)], args.rounds)
        ref = torch_nn(x, y)
        # torch's matrix is bf16: compare where its maximum is attained once, values within bf16 rounding
        agree = float((ref[1] == ri).float().mean())
        verr = float((ref[0].float() - rs).abs().max())
        flop = 2.0 * t * t * d * P
        print(json.dumps({"kernel": "nn_cosine", "workload": name, "pairs": P, "t": t, "d": d, "ms": round(ms, 4), "ms_min": round(ms_min, 4),
                          "torch_ms": round(tms, 4), "torch_ms_min": round(tms_min, 4), "torch_over_kernel": round(tms / ms, 3),
                          "TF_per_s": round(flop / ms / 1e9, 1), "share_of_bf16_peak": round(flop / (ms * 1e-3) / PEAK_BF16, 4),
                          "sim_matrix_MB_not_written": round(P * t * t * 4 / 1e6, 1), "steps_per_round": steps,
                          "row_idx_agree_with_torch_bf16": round(agree, 4), "max_abs_row_sim_diff": verr}), flush=True)
        del x, y, work, ref
        torch.cuda.empty_cache()
    if not args.e2e:
        return
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for size, stride, B in ((224, 16, 8), (224, 8, 8), (512, 8, 1)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        x1 = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        x2 = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()

        def two():
            model.extract_descriptors(x1, None, "key", bin=True)
            model.extract_descriptors(x2, None, "key", bin=True)

        (fc, ed), _, steps = interleaved([lambda: model.find_correspondences(x1, x2), two], args.rounds)
        print(json.dumps({"workload": "vit_base16", "size": size, "stride": stride, "grid": list(model.grid), "pairs": B,
                          "find_correspondences_ms": round(fc, 3), "two_extract_descriptors_ms": round(ed, 3),
                          "steps_per_round": steps}), flush=True)


if __name__ == "__main__":
    main()
