#!/usr/bin/env python3
"""Cost of the affinity-graph ops and of the spectral methods on top of them against the same quantities composed from torch
ops on the same bf16 inputs.

    python tools/spectral_bench.py [--rounds R] [--e2e 0|1] > profiles/spectral_bench.txt

One process, one device; shapes in ascending size; every shape's result is checked against torch BEFORE it is timed (a failed
check ends the run).  The sides alternate round by round (who goes first alternates too), device events around `steps` calls
after a warm call; per side the median over the rounds and the spread (min, max) are reported.  JSON lines, one per shape:
  affinity_bits_ms        vdr.ops.affinity_bits                      | torch: normalize (fp32) -> bf16, matmul, `>` (bool [t, t])
  matvec1_ms / matvec8_ms vdr.ops.bits_matvec, nv = 1 / 8            | torch: fp32 bmm with the materialised fp32 W = B
  fiedler_ms              vdr.spectral.fiedler end to end            | the same Lanczos (same code) with that dense bmm as product
At P > 1 with t >= 3969 the torch side multiplies problem by problem (mm in a loop): torch's batched bf16 bmm is recorded as
wrong there (profiles/correspondence_bench.txt).  A ratio below 1 is a loss and is printed as one.
Workload lines: model.tokencut on one ViT-B/16 handle against extract_descriptors + a host scipy.linalg.eigh of the same
generalised problem, at a threshold that gives a graph with both kinds of entries (asserted before timing); the Lanczos steps
taken, the residual and both sides' eigenvalues are recorded (the host graph is thresholded in float64 on fp32 descriptors, the
device graph in fp32 on bf16 ones: the eigenvalues agree only as far as that difference allows)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

SHAPES = ((64, 196, 768), (32, 729, 768), (1, 3969, 768), (1, 3969, 13056), (8, 3969, 768))
TAU = 0.2


def span_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, rounds, budget_ms=100.0):
    """(median, min, max) ms per call of each fn over `rounds` alternating rounds; steps per round sized from a first timed call"""
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
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def maps(P, t, d, seed):
    """planted maps on the device: noise + a_i times a shared direction (scores spread over [0, 0.8], tests/spectral_ref.py)"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(P, t, d, device="cuda", generator=gen)
    x += 2.0 * torch.rand(P, t, 1, device="cuda", generator=gen) * torch.randn(P, 1, d, device="cuda", generator=gen)
    return x.to(torch.bfloat16)


def torch_graph(x, loop):
    xn = torch.nn.functional.normalize(x.float(), dim=-1).to(torch.bfloat16)
    if loop:
        return torch.stack([(xn[p] @ xn[p].T) > TAU for p in range(x.shape[0])])
    return torch.bmm(xn, xn.transpose(1, 2)) > TAU


def bench_ops(rounds):
    from vdr import ops, spectral
    for P, t, d in SHAPES:
        loop = P > 1 and t >= 3969
        x = maps(P, t, d, t + d + P)
        bits = ops.affinity_bits(x, tau=TAU)
        B = ops.unpack_bits(bits, t)
        # ---- checks, before any timing
        xf = x.float()
        rn = 1.0 / xf.norm(dim=-1).clamp_min(1e-8)
        wrong, judged = 0, 0
        for p in range(P):  # fp32 scores problem by problem; entries further than 4e-3 from tau (above the fp32 bound at d = 13056) must agree
            s = (xf[p] @ xf[p].T) * (rn[p][:, None] * rn[p][None, :])
            clear = (s - TAU).abs() > 4e-3
            wrong += int((B[p] != (s > TAU))[clear].sum())
            judged += int(clear.sum())
        assert wrong == 0 and judged > 0.9 * P * t * t, ("affinity_bits disagrees with torch", P, t, d, wrong, judged)
        assert torch.equal(B, B.transpose(1, 2))
        tb = torch_graph(x, loop)
        bf16_agree = float((tb == B).float().mean())
        W = B.to(torch.float32)
        gen = torch.Generator(device="cuda").manual_seed(1)
        V1 = torch.randn(P, t, 1, device="cuda", generator=gen)
        V8 = torch.randn(P, t, 8, device="cuda", generator=gen)
        for V in (V1, V8):
            y, want = ops.bits_matvec(bits, V), torch.bmm(W.double(), V.double())
            lim = t * 2.0 ** -24 * torch.bmm(W.double(), V.double().abs())
            assert bool(((y.double() - want).abs() <= lim).all()), ("bits_matvec disagrees with torch", P, t, d)
        dense = lambda b_, v: torch.bmm(W, v.to(torch.float32).unsqueeze(-1))[..., 0].to(torch.float64)  # noqa: E731
        vec, val, resid, steps = spectral.fiedler(bits)
        dvec, dval, _, dsteps = spectral.fiedler(bits, product=dense)
        cos = (vec * dvec).sum(1).abs()
        assert float((val - dval).abs().max()) < 1e-4 and float((1 - cos).max()) < 1e-4, ("fiedler disagrees with the dense run", P, t, d)
        # ---- timing
        ms = interleaved([lambda: ops.affinity_bits(x, tau=TAU), lambda: torch_graph(x, loop),
                          lambda: ops.bits_matvec(bits, V1), lambda: torch.bmm(W, V1),
                          lambda: ops.bits_matvec(bits, V8), lambda: torch.bmm(W, V8),
                          lambda: spectral.fiedler(bits), lambda: spectral.fiedler(bits, product=dense)], rounds)
        r = lambda v: [round(q, 4) for q in v]  # noqa: E731
        ratio = lambda a, b: round(ms[b][0] / ms[a][0], 3)  # noqa: E731
        print(json.dumps({"kernel": "affinity", "P": P, "t": t, "d": d, "tau": TAU, "edge_share": round(float(W.mean()), 3),
                          "bits_MB": round(bits.numel() * 4 / 2 ** 20, 3), "dense_fp32_MB": round(W.numel() * 4 / 2 ** 20, 1),
                          "torch_side": "mm loop" if loop else "bmm", "agree_with_torch_bf16_graph": round(bf16_agree, 5),
                          "[median, min, max] ms": "every *_ms field",
                          "affinity_bits_ms": r(ms[0]), "torch_graph_ms": r(ms[1]), "torch_over_affinity_bits": ratio(0, 1),
                          "matvec1_ms": r(ms[2]), "torch_bmm1_ms": r(ms[3]), "torch_over_matvec1": ratio(2, 3),
                          "matvec8_ms": r(ms[4]), "torch_bmm8_ms": r(ms[5]), "torch_over_matvec8": ratio(4, 5),
                          "fiedler_steps": steps, "fiedler_resid_max": float(resid.max()), "fiedler_ms": r(ms[6]),
                          "fiedler_dense_product_ms": r(ms[7]), "dense_over_bits_fiedler": ratio(6, 7),
                          "fiedler_ms_per_step": round(ms[6][0] / steps, 4)}), flush=True)
        del x, xf, bits, B, W, tb
        torch.cuda.empty_cache()


def bench_e2e(rounds):
    import numpy as np
    import scipy.linalg
    import vdr
    from oracle import vit_oracle as vo
    from vdr import ops
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for stride in (16, 8):
        model.set_patch_stride(stride)
        x = torch.rand(4, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
        # The keys of a random-weight network share a large common component (every cosine is near 0.93): at tau = 0.2 the graph
        # is complete, Lanczos has nothing to do and stops at its first check.  The threshold of this workload is the median
        # cosine of image 0, so that every graph has both kinds of entries -- checked before anything is timed.
        d0 = torch.nn.functional.normalize(model.extract_descriptors(x, None, "key")[:, 0].double(), dim=-1)
        tau = float(torch.quantile((d0[0] @ d0[0].T).flatten(), 0.5))
        tc = model.tokencut(x, tau=tau)
        t = tc.bits.shape[1]
        shares = ops.unpack_bits(tc.bits, t).double().mean(dim=(1, 2))
        assert bool(((shares > 0.02) & (shares < 0.98)).all()), ("degenerate graph", stride, tau, shares.tolist())

        def host():
            d = model.extract_descriptors(x, None, "key")[:, 0]
            f = torch.nn.functional.normalize(d, dim=-1).double().cpu().numpy()
            vals = []
            for p in range(f.shape[0]):
                Wm = 1e-5 + (1 - 1e-5) * ((f[p] @ f[p].T) > tau)
                D = np.diag(Wm.sum(1))
                vals.append(scipy.linalg.eigh(D - Wm, D, subset_by_index=[1, 1], eigvals_only=False)[0][0])
            return vals

        host_vals = host()
        ms = interleaved([lambda: model.tokencut(x, tau=tau), host], rounds, budget_ms=40.0)
        print(json.dumps({"workload": "model.tokencut vit_base16 224^2 (random weights, tau = median cosine of image 0)",
                          "stride": stride, "images": 4, "grid": list(model.grid), "tau": round(tau, 5),
                          "edge_share": [round(float(v), 3) for v in shares], "fiedler_steps": tc.steps,
                          "fiedler_resid_max": float(tc.resid.max()), "eigval": [round(float(v), 6) for v in tc.eigval],
                          "host_eigval": [round(float(v), 6) for v in host_vals],
                          "[median, min, max] ms": "every *_ms field", "tokencut_ms": [round(q, 3) for q in ms[0]],
                          "extract_plus_scipy_eigh_host_ms": [round(q, 3) for q in ms[1]],
                          "host_over_tokencut": round(ms[1][0] / ms[0][0], 3)}), flush=True)
    model.set_patch_stride(16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
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
