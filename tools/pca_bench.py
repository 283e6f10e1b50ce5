#!/usr/bin/env python3
"""Cost of the PCA of dense descriptors: the three library ops (csrc/pca.hip) against the same quantities composed from
torch ops on the same inputs, the eigen-decomposition's share of vdr.pca.fit, and pca_descriptors end to end beside
extract_descriptors + sklearn on the host.

    python tools/pca_bench.py [--rounds R] [--e2e 0|1] > profiles/pca_bench.txt
    python tools/pca_bench.py --eigh-only > profiles/pca_eigh_bench.txt

One process, one device; the two sides alternate round by round (who goes first alternates too), device events around
`steps` calls after a warm-up; medians over the rounds.  Times are per call of an op, i.e. over all of its launches.
JSON lines per workload (problems x rows x d, dtype, per image or joint):
  mean        vdr_op_col_mean against x.float().mean(1); TB/s of the algorithmic bytes (the map read once)
  covariance  vdr_op_covariance against the centred Z^T Z through the vendor GEMM (centre in fp32, round to bf16, bmm of bf16
              with fp32 output, divide) -- TF/s of 2 R d^2 per problem -- and against the bmm alone on a ready-made Z
  project     vdr_op_pca_project (scale=False) against torch.matmul of the centred fp32 map, plus amin / amax; TB/s of the
              map read once and the projection written once
  fit         vdr.pca.fit, and the time and share of its eigen-decomposition (vdr.pca.components_from_covariance: one
              batched torch.linalg.eigh call in float64 plus the selection and sign rule)
  e2e lines   VitDescriptorModel.pca_descriptors(x) against extract_descriptors(x).cpu() followed by
              sklearn.decomposition.PCA(3).fit_transform per image on the host (skipped when sklearn is missing)
--eigh-only: torch.linalg.eigh in float64 by itself, per d in 256 / 768 / 2048: one call on the device and on the host, and
  16 problems (64 too at d = 768) as a loop of single device calls against one batched call; wall-clock ms around a
  synchronise, median of 3 after a warm-up."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

WORKLOADS = (("vit_base16 224^2 tokens, per image", 64, 196, 768, torch.bfloat16, False),
             ("vit_base16 224^2 tokens, joint", 64, 196, 768, torch.bfloat16, True),
             ("vit_base16 224^2 stride 8, per image", 16, 729, 768, torch.bfloat16, False),
             ("vit_base16 224^2 stride 8, joint", 16, 729, 768, torch.bfloat16, True),
             ("medsam neck, per image", 16, 4096, 256, torch.float32, False),
             ("medsam neck, joint", 16, 4096, 256, torch.float32, True),
             ("vit_base16 512^2 stride 8, one map", 1, 3969, 768, torch.bfloat16, False))


def span_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, rounds, budget_ms=100.0):
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
    return [sorted(t)[len(t) // 2] for t in times]


def wall_ms(fn, sync):
    fn()
    ts = []
    for _ in range(3):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[1], 3)


def eigh_only():
    for d, batches in ((256, (16,)), (768, (16, 64)), (2048, (16,))):
        gen = torch.Generator().manual_seed(d)
        for B in batches:
            a = torch.randn(B, d, 300, dtype=torch.float64, generator=gen)
            c = (a @ a.transpose(1, 2) / 299).cuda()
            host = c[0].cpu()
            print(json.dumps({"eigh": "float64", "d": d, "problems": B,
                              "one_device_call_ms": wall_ms(lambda: torch.linalg.eigh(c[0]), True),
                              "one_host_call_ms": wall_ms(lambda: torch.linalg.eigh(host), False),
                              "loop_of_device_calls_ms": wall_ms(lambda: [torch.linalg.eigh(m) for m in c], True),
                              "one_batched_device_call_ms": wall_ms(lambda: torch.linalg.eigh(c), True)}), flush=True)
            del c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--e2e", type=int, default=1)
    ap.add_argument("--eigh-only", action="store_true")
    args = ap.parse_args()
    import vdr
    from vdr import ops, pca
    torch.cuda.set_device(0)
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds}), flush=True)
    if args.eigh_only:
        return eigh_only()
    for name, P, t, d, dtype, joint in WORKLOADS:
        gen = torch.Generator(device="cuda").manual_seed(t + d)
        x = (torch.randn(P, t, d, device="cuda", generator=gen) * 2 + torch.randn(d, device="cuda", generator=gen)).to(dtype)
        xs = x.reshape(1, P * t, d) if joint else x  # what the torch side sees
        problems, R = xs.shape[0], xs.shape[1]
        esz = x.element_size()
        mean, cov = ops.covariance(x, None, joint)
        comps = pca.components_from_covariance(cov, 3)[0]
        z = (xs.float() - mean.unsqueeze(1)).to(torch.bfloat16)

        def t_cov():
            zz = (xs.float() - mean.unsqueeze(1)).to(torch.bfloat16)
            return torch.bmm(zz.transpose(1, 2), zz, out_dtype=torch.float32) / (R - 1)

        def t_bmm():
            return torch.bmm(z.transpose(1, 2), z, out_dtype=torch.float32)

        def t_proj():
            pr = torch.matmul(xs.float() - mean.unsqueeze(1), comps.transpose(1, 2))
            return pr, pr.amin(dim=(1, 2)), pr.amax(dim=(1, 2))

        try:
            t_bmm()
        except (TypeError, RuntimeError):  # (a torch without bmm(out_dtype=): fp32 operands through the vendor GEMM)
            def t_cov():  # noqa: F811
                zz = (xs.float() - mean.unsqueeze(1)).to(torch.bfloat16).float()
                return torch.bmm(zz.transpose(1, 2), zz) / (R - 1)

            def t_bmm():  # noqa: F811
                return torch.bmm(z.float().transpose(1, 2), z.float())

        m_ms, tm_ms = interleaved([lambda: ops.col_mean(x, joint), lambda: xs.float().mean(1)], args.rounds)
        c_ms, tc_ms, tb_ms = interleaved([lambda: ops.covariance(x, mean, joint), t_cov, t_bmm], args.rounds)
        p_ms, tp_ms = interleaved([lambda: ops.pca_project(x, mean, comps), t_proj], args.rounds)
        f_ms, e_ms = interleaved([lambda: pca.fit(x, 3, joint), lambda: pca.components_from_covariance(cov, 3)], args.rounds)
        err = float((t_cov() - cov).abs().max() / cov.abs().max())
        flop = 2.0 * R * d * d * problems
        print(json.dumps({"workload": name, "problems": problems, "R": R, "d": d, "dtype": str(dtype).split(".")[1],
                          "mean_ms": round(m_ms, 4), "torch_mean_ms": round(tm_ms, 4), "mean_TB_per_s": round(P * t * d * esz / m_ms / 1e9, 3),
                          "cov_ms": round(c_ms, 4), "torch_centre_bmm_ms": round(tc_ms, 4), "torch_bmm_only_ms": round(tb_ms, 4),
                          "cov_TF_per_s": round(flop / c_ms / 1e9, 1), "torch_cov_TF_per_s": round(flop / tc_ms / 1e9, 1),
                          "torch_over_kernel_cov": round(tc_ms / c_ms, 3), "cov_rel_diff_to_torch": err,
                          "project_ms": round(p_ms, 4), "torch_project_minmax_ms": round(tp_ms, 4),
                          "project_TB_per_s": round((P * t * d * esz + P * t * 3 * 4) / p_ms / 1e9, 3),
                          "fit_ms": round(f_ms, 3), "eigh_ms": round(e_ms, 3), "eigh_share_of_fit": round(e_ms / f_ms, 3)}), flush=True)
        del x, xs, z, cov
        torch.cuda.empty_cache()
    if not args.e2e:
        return
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        PCA = None
    from oracle import vit_oracle as vo
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for size, stride, B in ((224, 16, 16), (224, 8, 16), (512, 8, 1)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        x = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        pd, ed = interleaved([lambda: model.pca_descriptors(x, facet="key"), lambda: model.extract_descriptors(x, facet="key")], args.rounds)
        row = {"workload": "vit_base16 key facet", "size": size, "stride": stride, "grid": list(model.grid), "batch": B,
               "pca_descriptors_ms": round(pd, 3), "extract_descriptors_ms": round(ed, 3)}
        if PCA is not None:
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = model.extract_descriptors(x, facet="key")[:, 0].cpu().numpy()
                for b in range(B):
                    PCA(n_components=3).fit_transform(f[b])
                host.append((time.perf_counter() - t0) * 1e3)
            row["extract_descriptors_plus_host_sklearn_ms"] = round(sorted(host)[1], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
