#!/usr/bin/env python3
"""Cost of the k-means of dense descriptors: vdr_op_kmeans_assign, vdr_op_kmeans_update, one Lloyd iteration and a whole
vdr.kmeans.fit against the same quantities composed from torch ops on the same bf16 inputs -- the assignment as
cc - 2 x c^T by matmul (which materialises the [R, k] matrix) + argmin, the update as index_add_ + bincount + a division --
and cosegment / points(select="kmeans") end to end against extract_descriptors + sklearn.cluster.KMeans on the host.

    python tools/kmeans_bench.py [--rounds R] [--e2e 0|1] > profiles/kmeans_bench.txt

One process, one device; the sides alternate round by round (who goes first alternates too), device events around `steps`
calls after a warm-up; medians over the rounds.  Maps are planted-cluster maps (k centres, unit noise) made on the device.
JSON lines:
  kernel "kmeans": workload, problems, imgs, t, d, k; assign / update / iteration ms beside torch's, the ratios; the fit (init
      "first", the iterations it took, ms with sync_every 16 and 0) beside a torch loop of the same number of iterations with
      no host read; labels_agree: the share of rows on which the two assignments agree.
  "launch_floor": the same five launches + one torch op per iteration on a 128 x 32 map, k = 2: what an iteration costs when
      the kernels have nothing to do -- an iteration that costs about this much is bound by launch gaps, not by its kernels.
  workload lines: cosegment(k=10) and points(num_pairs=10, select="kmeans") on one ViT-B/16 handle against the same
      descriptors taken to the host and clustered by sklearn (n_init=1, the same number of clusters), ms per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

#            name                                      problems imgs t     d      k
WORKLOADS = (("vit_base16 224^2 keys, joint over 8",    1,       8,   196,  768,   10),
             ("vit_base16 224^2 stride 8, joint over 8", 1,      8,   729,  768,   10),
             ("vit_base16 224^2 binned h=2, per image", 8,       1,   196,  13056, 10),
             ("buddies map (2 x binned)",               1,       1,   150,  26112, 10))


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
    steps = [max(1, min(50, int(budget_ms / max(t, 1e-3)))) for t in first]
    times = [[] for _ in fns]
    for r in range(rounds):
        order = range(len(fns)) if r & 1 else reversed(range(len(fns)))
        for i in order:
            times[i].append(span_ms(fns[i], steps[i]))
    return [sorted(t)[len(t) // 2] for t in times]


def torch_assign(xf, c):
    """xf [problems, R, d] bf16, c [problems, k, d] fp32 -> (labels, min_dist): bf16 matmul against the rounded centroids, as a
    torch user would write it"""
    h = (c * c).sum(-1).unsqueeze(1) - 2.0 * torch.bmm(xf, c.to(torch.bfloat16).transpose(1, 2)).float()
    v, i = h.min(dim=-1)
    return i, (v + (xf.float() ** 2).sum(-1)).clamp_min(0)


def torch_update(xf, labels, c):
    P, k, d = c.shape
    sums = torch.zeros_like(c)
    counts = torch.zeros(P, k, device=c.device)
    for p in range(P):
        sums[p].index_add_(0, labels[p], xf[p].float())
        counts[p] = torch.bincount(labels[p], minlength=k).float()
    return torch.where(counts.unsqueeze(-1) > 0, sums / counts.clamp_min(1).unsqueeze(-1), c)


def planted(problems, imgs, t, d, k, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(problems, k, d, device="cuda", generator=gen) * 0.3
    lab = torch.randint(0, k, (problems, imgs * t), device="cuda", generator=gen)
    x = torch.gather(centres, 1, lab.unsqueeze(-1).expand(-1, -1, d)) + torch.randn(problems, imgs * t, d, device="cuda", generator=gen)
    return x.to(torch.bfloat16).reshape(problems, imgs, t, d)


def bench_ops(rounds):
    from vdr import kmeans, ops
    for name, P, imgs, t, d, k in WORKLOADS + (("launch_floor", 1, 1, 128, 32, 2),):
        x = planted(P, imgs, t, d, k, t + d)
        o = ops.kmeans_operand(x)
        xf = x.reshape(P, imgs * t, d)
        c0 = xf[:, :k].float().contiguous()
        work = o.work(k)
        labels = torch.full((P, o.R), -1, dtype=torch.int32, device="cuda")
        out = (torch.empty(P, o.R, device="cuda"), torch.empty(P, device="cuda"), torch.empty(P, dtype=torch.int32, device="cuda"))
        counts = torch.zeros(P, k, dtype=torch.int32, device="cuda")
        cent = c0.clone()
        ops.kmeans_assign(o, c0, labels, out=out, work=work)
        tl, _ = torch_assign(xf, c0)
        agree = float((tl == labels).float().mean())
        tl = tl.contiguous()

        def assign():
            ops.kmeans_assign(o, c0, labels, out=out, work=work)

        def update():
            ops.kmeans_update(o, labels, cent, inplace=True, counts=counts, work=work)

        def iteration():
            assign()
            update()

        def t_iteration():
            torch_update(xf, torch_assign(xf, c0)[0], c0)

        res = kmeans.fit(xf if imgs == 1 else xf.reshape(imgs, t, d), k, init="first", joint=imgs > 1)
        iters = int(res.iters.max())

        def fit16():
            kmeans.fit(xf if imgs == 1 else xf.reshape(imgs, t, d), k, init="first", joint=imgs > 1)

        def fit0():
            kmeans.fit(xf if imgs == 1 else xf.reshape(imgs, t, d), k, init="first", joint=imgs > 1, sync_every=0, max_iter=iters)

        def t_fit():
            c = c0
            for _ in range(iters):
                c = torch_update(xf, torch_assign(xf, c)[0], c)

        ms = interleaved([assign, lambda: torch_assign(xf, c0), update, lambda: torch_update(xf, tl, c0), iteration, t_iteration,
                          fit16, fit0, t_fit], rounds)
        r = lambda v: round(v, 4)  # noqa: E731
        line = {"kernel": "kmeans", "workload": name, "problems": P, "imgs": imgs, "t": t, "d": d, "k": k,
                "assign_ms": r(ms[0]), "torch_assign_ms": r(ms[1]), "torch_over_assign": round(ms[1] / ms[0], 3),
                "update_ms": r(ms[2]), "torch_update_ms": r(ms[3]), "torch_over_update": round(ms[3] / ms[2], 3),
                "iteration_ms": r(ms[4]), "torch_iteration_ms": r(ms[5]), "torch_over_iteration": round(ms[5] / ms[4], 3),
                "fit_iters": iters, "converged": bool(res.converged.all()), "fit_ms_sync16": r(ms[6]), "fit_ms_sync0": r(ms[7]),
                "torch_loop_ms": r(ms[8]), "torch_over_fit": round(ms[8] / ms[7], 3), "fit_ms_per_iter": r(ms[7] / iters),
                "labels_agree_with_torch_bf16": round(agree, 4)}
        if name == "launch_floor":
            line = {"launch_floor": True, **{f: line[f] for f in ("t", "d", "k", "assign_ms", "update_ms", "iteration_ms", "fit_iters",
                                                                     "fit_ms_per_iter")}}
        print(json.dumps(line), flush=True)
        del x, xf, work
        torch.cuda.empty_cache()


def bench_e2e(rounds):
    import vdr
    from oracle import vit_oracle as vo
    from sklearn.cluster import KMeans
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    for stride in (16, 8):
        model.set_patch_stride(stride)
        x1 = torch.rand(8, 3, 224, 224).to(torch.bfloat16).cuda()
        x2 = torch.rand(8, 3, 224, 224).to(torch.bfloat16).cuda()

        def host_coseg():
            d = model.extract_descriptors(x1, None, "key")[:, 0]
            rows = torch.nn.functional.normalize(d, dim=-1).reshape(-1, d.shape[-1]).cpu().numpy()
            KMeans(n_clusters=10, n_init=1, init="random", random_state=0).fit(rows)

        seg = model.cosegment(x1, k=10)
        ms = interleaved([lambda: model.cosegment(x1, k=10), host_coseg], rounds, budget_ms=60.0)
        print(json.dumps({"workload": "cosegment vit_base16 224^2", "stride": stride, "images": 8, "grid": list(model.grid), "k": 10,
                          "fit_iters": int(seg.kmeans.iters[0]), "cosegment_ms": round(ms[0], 3),
                          "extract_plus_sklearn_host_ms": round(ms[1], 3)}), flush=True)
        c = model.find_correspondences(x1, x2, thresh=-1.0, keep_descriptors=True)
        n_bb = int(c.mask[0].sum())
        if n_bb < 10:
            print(json.dumps({"workload": "points(select=kmeans)", "stride": stride, "skipped": f"{n_bb} buddies"}), flush=True)
            continue

        def host_points():
            idx, desc = c.buddy_descriptors(0)
            KMeans(n_clusters=10, n_init=1, init="random", random_state=0).fit(desc.float().cpu().numpy())

        ms = interleaved([lambda: c.points(0, 10, select="kmeans"), host_points], rounds, budget_ms=60.0)
        print(json.dumps({"workload": "points(select=kmeans) vit_base16 224^2 binned", "stride": stride, "buddies": n_bb,
                          "d": int(c.desc1.shape[-1]) * 2, "points_kmeans_ms": round(ms[0], 3),
                          "buddy_descriptors_plus_sklearn_host_ms": round(ms[1], 3)}), flush=True)
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
