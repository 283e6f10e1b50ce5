#!/usr/bin/env python3
"""Cost of the global k-nearest-neighbour search: vdr.ops.knn (all three launches) at k = 1 / 5 / 16, cosine and l2, against
  * this checkout's vdr.ops.nn_cosine(mutual=False) on the same inputs -- the same tile loop with the top-1 epilogue, so the
    difference is what the lists cost --, and
  * the same quantity from torch ops: normalize + mm + topk (cosine), ss + ss' - 2 mm + topk (l2), bf16 operands.  For more
    than one problem this is a per-problem mm loop, never a batched bmm (profiles/correspondence_bench.txt records wrong
    results from torch's batched bf16 bmm at 8 x 3969 on this build).

    python tools/knn_bench.py [--rounds R] > profiles/knn_bench.txt

The shapes form a ladder, ascending.  Every rung runs in a FRESH child process under its own time limit, and the ladder ends
at the first rung whose process does not exit with 0: nothing is started on a device after a fault.  The parent never opens
the device.  Before anything is timed a rung checks
  * the indices against vdr.knn.topk_dense on the device (per problem, first and last one) on the rows whose first k + 1
    costs are further apart than 4 d 2^-24 times the scale of the scores -- the share of such rows is printed --, and
  * the bits of the multi-problem run against one-problem runs of its first and last problem.
The last rung, 8 x 3969 x 3969 x 768, is the shape at which the benchmark of an earlier kernel died.  Its process
calls nothing but this library's kernels: the inputs are drawn on the host and copied, its check is the one-pair run compared
on the host, and there is no torch yardstick.
Timing: the sides alternate round by round, device events around `steps` calls after a warm-up, medians over the rounds
(correspondence_bench.interleaved).  JSON lines, ms per call; *_over_knn above 1 is a win for the kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# name, pairs, tq, tc, d, exclude_diag, time limit of the child in seconds
LADDER = (("64x196", 64, 196, 196, 768, False, 150), ("32x729", 32, 729, 729, 768, False, 150), ("1x3969", 1, 3969, 3969, 768, False, 150),
          ("classifier 1024 vs 65536", 1, 1024, 65536, 768, False, 240), ("cls graph 8192", 1, 8192, 8192, 384, True, 240),
          ("end to end", 0, 0, 0, 0, False, 300),
          ("8x3969 (library kernels only)", 8, 3969, 3969, 768, False, 240))
KS = (1, 5, 16)
METRICS = ("cosine", "l2")


def torch_topk(x, y, k, metric, diag):
    """what a user runs without the kernel, problem by problem"""
    import torch
    vals, idxs = [], []
    if metric == "cosine":
        xn = torch.nn.functional.normalize(x.float(), dim=-1).to(torch.bfloat16)
        yn = torch.nn.functional.normalize(y.float(), dim=-1).to(torch.bfloat16)
    else:
        ssx, ssy = (x.float() ** 2).sum(-1), (y.float() ** 2).sum(-1)
    for p in range(x.shape[0]):
        if metric == "cosine":
            s = (xn[p] @ yn[p].T).float()
        else:
            s = (ssx[p][:, None] + ssy[p][None, :] - 2.0 * (x[p] @ y[p].T).float()).clamp_min(0.0)
        if diag:
            s.fill_diagonal_(float("-inf") if metric == "cosine" else float("inf"))
        v, i = s.topk(k, dim=-1, largest=metric == "cosine")
        vals.append(v)
        idxs.append(i)
    return torch.stack(vals), torch.stack(idxs)


def check_against_dense(ops, knn, x, y, k, metric, diag):
    """indices against topk_dense on the rows with clear margins, problem by problem; returns the share of such rows"""
    import torch
    d = x.shape[-1]
    shares = []
    for p in sorted({0, x.shape[0] - 1}):
        val, idx = ops.knn(x[p:p + 1], y[p:p + 1], k, metric, diag)
        kk = min(k + 1, y.shape[1] - int(diag))
        kk = min(kk, 16)
        dv, di = knn.topk_dense(x[p:p + 1], y[p:p + 1], kk, metric, diag)
        scale = 1.0 if metric == "cosine" else 4.0 * float((y[p].float() ** 2).sum(-1).max())
        tol = 4.0 * d * 2.0 ** -24 * scale
        gaps = (dv[..., 1:] - dv[..., :-1]).abs()
        clear = (gaps > 2 * tol).all(-1) if kk > 1 else torch.ones_like(dv[..., 0], dtype=torch.bool)
        kc = min(k, kk)
        assert torch.equal(idx[..., :kc][clear], di[..., :kc][clear]), f"indices differ from topk_dense on clear rows ({metric}, k={k}, problem {p})"
        assert float((val[..., :kc] - dv[..., :kc]).abs().max()) <= tol, f"values differ from topk_dense ({metric}, k={k}, problem {p})"
        shares.append(float(clear.float().mean()))
    return min(shares)


def check_batch_bits(ops, x, y, k, metric, diag, to_host=False):
    """the multi-problem run against one-problem runs of its first and last problem, bit for bit"""
    import torch
    val, idx = ops.knn(x, y, k, metric, diag)
    for p in sorted({0, x.shape[0] - 1}):
        v1, i1 = ops.knn(x[p:p + 1], y[p:p + 1], k, metric, diag)
        if to_host:
            ok = torch.equal(val[p].cpu(), v1[0].cpu()) and torch.equal(idx[p].cpu(), i1[0].cpu())
        else:
            ok = torch.equal(val[p], v1[0]) and torch.equal(idx[p], i1[0])
        assert ok, f"problem {p} of {x.shape[0]} differs from its one-problem run ({metric}, k={k})"
    return val, idx


def rung(i, rounds):
    import torch
    import vdr
    from correspondence_bench import interleaved
    from vdr import _lib, knn, ops
    name, P, tq, tc, d, diag, _ = LADDER[i]
    torch.cuda.set_device(0)
    head = {"rung": name, "source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": rounds}
    if name == "end to end":
        return end_to_end(head, rounds)
    only_library = name.startswith("8x3969")
    gen = torch.Generator().manual_seed(tq + tc + d)
    # planted clusters on the host (7 centres, noise 0.5: the neighbours mean something), copied to the device
    centres = torch.randn(7, d, generator=gen)
    x = (centres[torch.randint(0, 7, (P, tq), generator=gen)] + 0.5 * torch.randn(P, tq, d, generator=gen)).to(torch.bfloat16).cuda()
    y = x if diag else (centres[torch.randint(0, 7, (P, tc), generator=gen)] + 0.5 * torch.randn(P, tc, d, generator=gen)).to(torch.bfloat16).cuda()
    out = dict(head, pairs=P, tq=tq, tc=tc, d=d, exclude_diag=diag, work_MB_k16=round(_lib.load().vdr_knn_work_bytes(P, tq, tc, 16) / 1e6, 1))
    # ---- checked before it is timed
    for metric in METRICS:
        for k in KS:
            val, idx = check_batch_bits(ops, x, y, k, metric, diag, to_host=only_library)
            if not only_library:
                out[f"clear_share_{metric}_k{k}"] = round(check_against_dense(ops, knn, x, y, k, metric, diag), 4)
    if not diag:
        rs, ri, _, _ = ops.nn_cosine(x, y, mutual=False)
        v1, i1 = ops.knn(x, y, 1)
        assert torch.equal(v1[..., 0].cpu(), rs.cpu()) and torch.equal(i1[..., 0].cpu(), ri.cpu()), "k = 1 differs from nn_cosine"
    out["checks"] = "passed"
    fns, names = [], []
    for metric in METRICS:
        for k in KS:
            fns.append(lambda k=k, metric=metric: ops.knn(x, y, k, metric, diag))
            names.append(f"knn_{metric}_k{k}")
    fns.append(lambda: ops.nn_cosine(x, y, mutual=False))
    names.append("nn_cosine")
    if not only_library:
        for metric in METRICS:
            fns.append(lambda metric=metric: torch_topk(x, y, 16, metric, diag))
            names.append(f"torch_{metric}_k16")
    med, mins, steps = interleaved(fns, rounds, budget_ms=100.0)
    for n, m, lo in zip(names, med, mins):
        out[n + "_ms"], out[n + "_ms_min"] = round(m, 4), round(lo, 4)
    t = dict(zip(names, med))
    for metric in METRICS:
        for k in KS:
            out[f"lists_cost_{metric}_k{k}_over_nn_cosine"] = round(t[f"knn_{metric}_k{k}"] / t["nn_cosine"], 3)
        if not only_library:
            out[f"torch_{metric}_k16_over_knn"] = round(t[f"torch_{metric}_k16"] / t[f"knn_{metric}_k16"], 3)
    out["executed_TF_per_s_cosine_k16"] = round(2.0 * P * (-(-tq // 128) * 128) * (-(-tc // 128) * 128) * d / t["knn_cosine_k16"] / 1e9, 1)
    out["steps_per_round"] = steps
    print(json.dumps(out), flush=True)


def end_to_end(head, rounds):
    """fit_knn + knn_predict beside linear_probe_features + a host k-NN; transfer_labels beside propagate_labels(radius=4)"""
    import torch
    import vdr
    from correspondence_bench import interleaved
    from oracle import vit_oracle as vo
    from vdr import knn
    try:
        from sklearn.neighbors import KNeighborsClassifier
    except ImportError:
        KNeighborsClassifier = None
    cfg = vo.VitCfg()
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(cfg, seed=1, scale=0.02))
    B, N = 16, 256
    gen = torch.Generator().manual_seed(3)
    bank = [torch.rand(B, 3, 224, 224, generator=gen).to(torch.bfloat16).cuda() for _ in range(N // B)]
    labels = torch.randint(0, 10, (N,), generator=gen)
    xq = torch.rand(B, 3, 224, 224, generator=gen).to(torch.bfloat16).cuda()

    def ours():
        return model.knn_predict(xq, model.fit_knn(bank, labels, 10, k=10))

    def host():
        f = torch.cat([model.linear_probe_features(b, 1, False) for b in bank]).cpu()
        q = model.linear_probe_features(xq, 1, False).cpu()
        if KNeighborsClassifier is not None:
            return KNeighborsClassifier(n_neighbors=10, algorithm="brute", metric="cosine").fit(f.numpy(), labels.numpy()).predict_proba(q.numpy())
        return knn.KnnClassifier(f, labels, 10, k=10, weights="uniform", backend="torch").predict_proba(q)

    (a, b), _, steps = interleaved([ours, host], rounds, budget_ms=400.0)
    print(json.dumps(dict(head, workload="vit_base16 k-NN classifier", bank=N, batch=B, fit_knn_plus_knn_predict_ms=round(a, 3),
                          host_yardstick="sklearn" if KNeighborsClassifier is not None else "vdr.knn torch backend on the CPU (no sklearn here)",
                          linear_probe_features_plus_host_knn_ms=round(b, 3), host_over_ours=round(b / a, 3), steps_per_round=steps)), flush=True)
    for size, stride, Bp in ((224, 16, 8), (224, 8, 8)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        grid = tuple(model.grid)
        x1 = torch.rand(Bp, 3, size, size, generator=gen).to(torch.bfloat16).cuda()
        x2 = torch.rand(Bp, 3, size, size, generator=gen).to(torch.bfloat16).cuda()
        lab = torch.randint(0, 4, (Bp,) + grid, generator=gen).cuda()
        (g, w), _, steps = interleaved([lambda: model.transfer_labels(x1, lab, x2, 4, k=5),
                                        lambda: model.propagate_labels(x1, lab, x2, 4, radius=4, k=5)], rounds, budget_ms=400.0)
        print(json.dumps(dict(head, workload="vit_base16 label transfer", size=size, stride=stride, grid=list(grid), pairs=Bp,
                              transfer_labels_k5_ms=round(g, 3), propagate_labels_radius4_k5_ms=round(w, 3),
                              global_over_window=round(g / w, 3), steps_per_round=steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rung", type=int, default=None, help="run this rung in this process (what the parent starts)")
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--last", type=int, default=len(LADDER) - 1)
    args = ap.parse_args()
    if args.rung is not None:
        return rung(args.rung, args.rounds)
    for i in range(args.first, args.last + 1):
        limit = LADDER[i][6]
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--rung", str(i), "--rounds", str(args.rounds)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"rung": LADDER[i][0], "exit": rc, "ladder": "ended here: nothing further is started"}), flush=True)
            sys.exit(1)
    print(json.dumps({"ladder": "complete", "rungs": args.last - args.first + 1}), flush=True)


if __name__ == "__main__":
    main()
