#!/usr/bin/env python3
"""Cost of the anomaly score of dense descriptors: vdr_op_mahalanobis against the same distances from torch ops on the same
inputs, ((x.float() - mean) @ W.T).square().sum(-1), which writes the [rows, k] whitened matrix in fp32 -- and
model.anomaly_map end to end against extract_descriptors plus that expression.

    python tools/anomaly_bench.py [--rounds R] [--e2e 0|1] > profiles/anomaly_bench.txt

One process, one device; the sides alternate round by round (who goes first alternates too), device events around `steps`
calls after a warm-up; medians over the rounds.  Every shape is checked against the fp32 torch expression before it is timed
(worst relative difference printed; above 1e-4 the tool stops).  Maps are planted-spectrum maps made on the device, the model
is fitted on them by vdr.anomaly.fit_gaussian (shrinkage 0.01).
JSON lines:
  kernel "mahalanobis": workload, problems, R (rows per problem), d, k, items (workgroups: problems x 128-row panels),
      tile_rows_filled (the share of the staged panel rows that are real), mahalanobis_ms, torch_ms, torch_over_vdr,
      tflops (2 * rows * k * d * 3 products / time: the MFMA work the kernel does), worst_rel (against torch).
  workload lines: anomaly_map on one ViT-B/16 handle against extract_descriptors + the torch expression, ms per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

#            name                                          B    t     d    k     per_position
WORKLOADS = (("vit_base16 224^2 keys, 64 images",          64,  196,  768, 768,  False),
             ("vit_base16 224^2 keys, 64 images, k = 128", 64,  196,  768, 128,  False),
             ("vit_base16 224^2 stride 8, 32 images",      32,  729,  768, 768,  False),
             ("vit_base16 448^2 stride 7, 1 image",        1,   3969, 768, 768,  False),
             ("per position (PaDiM), 8 images",            8,   196,  768, 128,  True))


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


def planted(B, t, d, seed):
    """[B, t, d] bf16 on the device: rows N(mu, Q diag(s) Q^T), s log-spaced over two decades"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn((d, d), generator=gen, device="cuda"))
    s = torch.logspace(0.0, -2.0, d, device="cuda").sqrt()
    z = torch.randn((B * t, d), generator=gen, device="cuda") * s
    return (z @ q.T + 0.5).reshape(B, t, d).to(torch.bfloat16)


def torch_d2(x, mean, w):
    """x [P, R, d] bf16, mean [P, d] (or [1, d]), w [P, k, d] (or [1, k, d]) fp32 -> [P, R]"""
    return ((x.float() - mean.unsqueeze(1)) @ w.transpose(1, 2)).square().sum(-1)


def bench_ops(rounds):
    from vdr import anomaly
    for name, B, t, d, k, pos in WORKLOADS:
        x = planted(B, t, d, seed=B + t)
        train = planted(16 if pos else max(2, -(-2 * d // t)), t, d, seed=7)  # (global: at least 2 d rows; per position: 16 each)
        g = anomaly.fit_gaussian(train, per_position=pos, shrinkage=0.01, n_components=k)
        del train
        if pos:
            xt = x.transpose(0, 1)  # [t, B, d]: position p is problem p
            ref = lambda: torch_d2(xt, g.mean, g.whiten).t()  # noqa: E731
            problems, R = t, B
        else:
            ref = lambda: torch_d2(x, g.mean, g.whiten)  # noqa: E731
            problems, R = B, t
        got, want = g.score(x), ref()
        rel = float(((got - want).abs() / want).max())
        panels = (R + 127) // 128
        line = {"kernel": "mahalanobis", "workload": name, "problems": problems, "R": R, "d": d, "k": k,
                "items": problems * panels, "tile_rows_filled": round(R / (128 * panels), 3), "worst_rel": float(f"{rel:.3e}")}
        if not rel <= 1e-4:
            print(json.dumps(dict(line, error="differs from the fp32 torch expression")), flush=True)
            sys.exit(1)
        ms = interleaved([lambda: g.score(x), ref], rounds)
        line.update(mahalanobis_ms=round(ms[0], 4), torch_ms=round(ms[1], 4), torch_over_vdr=round(ms[1] / ms[0], 3),
                    tflops=round(6.0 * problems * R * k * d / (ms[0] * 1e9), 1))
        print(json.dumps(line), flush=True)


def bench_e2e(rounds):
    import vdr
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for stride, B in ((16, 64), (8, 32)):
        model.set_patch_stride(stride)
        normal = [torch.rand(B, 3, 224, 224).to(torch.bfloat16).cuda() for _ in range(2)]
        x = torch.rand(B, 3, 224, 224).to(torch.bfloat16).cuda()
        for pos in (False, True):
            if pos and stride != 16:
                continue  # (729 covariances of 768 x 768 in float64 are 3.4 GB per copy: the per-position fit is for the coarse grid)
            g = model.fit_anomaly(normal, per_position=pos, shrinkage=0.01, n_components=128 if pos else None)

            def composed():
                d = model.extract_descriptors(x, None, "key")[:, 0]
                if pos:
                    return torch_d2(d.transpose(0, 1), g.mean, g.whiten).t()
                return torch_d2(d, g.mean, g.whiten)

            got, want = model.anomaly_map(x, g).d2.reshape(B, -1), composed()
            rel = float(((got - want).abs() / want).max())
            ms = interleaved([lambda: model.anomaly_map(x, g), composed], rounds, budget_ms=100.0)
            print(json.dumps({"workload": "anomaly_map vit_base16 224^2 keys", "stride": stride, "images": B, "grid": list(model.grid),
                              "per_position": pos, "k": int(g.whiten.shape[1]), "worst_rel": float(f"{rel:.3e}"),
                              "anomaly_map_ms": round(ms[0], 3), "extract_plus_torch_ms": round(ms[1], 3),
                              "torch_over_vdr": round(ms[1] / ms[0], 3)}), flush=True)
    model.set_patch_stride(16)


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
