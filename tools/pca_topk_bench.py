#!/usr/bin/env python3
"""vdr.pca.fit(solver="subspace") -- the library's top-k eigensolver on the smaller side -- against the default eigh route,
in one process, the two alternating round by round (tools/pca_bench.py's `interleaved`): the yardstick is the eigh route
of the same checkout, measured here.

    python tools/pca_topk_bench.py [--rounds R] [--e2e 0|1] > profiles/pca_topk_bench.txt

JSON lines:
  fit     per workload of the README's PCA table (tools/pca_bench.py WORKLOADS), on two kinds of input: "white" -- the
          table's own white-noise maps, whose covariance has NO falling spectrum (the worst case for any iteration: the
          solver runs into max_iter and fit falls back to eigh, with a warning) -- and "decay" -- the same shapes with a
          planted spectrum lambda_j = 0.7^j over white noise 1e-3 below, what a descriptor map looks like.  Both solvers'
          ms per fit, the side taken, the iterations used, the worst residual, how many problems fell back; and the ms of one
          iteration (all three launches: sym_topk with tol = 0 at 20 iterations minus at 1, over 19) with the bytes of A read
          once over that time as TB/s -- what the A V kernel would reach if the iteration were nothing else (HBM peak: 8 TB/s)
  binned  one log-binned map, 196 x 13 056 and 729 x 13 056 bf16 (Gram side only: the default route refuses the width)
  e2e     pca_descriptors (eigh) against pca_descriptor_maps(solver="subspace") on vit_base16 key facets: 16 images at 224^2,
          16 at stride 8, one 512^2 image at stride 8 -- and the binned facet with the subspace solver alone
  iters   (kind = golden / model / white noise) the iterations fit(solver="subspace") needs with max_iter out of the way: the
          golden sklearn maps, vit_base16 key facets per image, joint and log-binned at the three e2e sizes, two white-noise
          maps (VDR_TOPK_MAX_ITER is twice the largest count of a golden map or a model workload)
  tol     the residual floor on planted spectra: sym_topk(tol=0) after 5 .. 80 iterations (VDR_TOPK_TOL is four times the worst
          level at which it stops falling)."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "vit-deep-radiomics_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from tools.pca_bench import WORKLOADS, interleaved  # noqa: E402


def make_map(kind, P, t, d, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    noise = torch.randn(P, t, d, device="cuda", generator=gen)
    offset = torch.randn(d, device="cuda", generator=gen)
    if kind == "white":
        return (noise * 2 + offset).to(dtype)
    r = min(t, d, 48)
    lam = 0.7 ** torch.arange(r, device="cuda", dtype=torch.float32)
    basis = torch.linalg.qr(torch.randn(d, r, device="cuda", generator=gen))[0]
    coef = torch.randn(P, t, r, device="cuda", generator=gen) * lam.sqrt()
    return (coef @ basis.t() * 4 + noise * (4 * 1e-3 ** 0.5) + offset).to(dtype)


def fit_rows(args, vdr, ops, pca):
    for name, P, t, d, dtype, joint in WORKLOADS:
        for kind in ("white", "decay"):
            x = make_map(kind, P, t, d, dtype, t + d)
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                p = pca.fit(x, 3, joint, "subspace")
                fell_back = int((~(p.resid <= ops.TOPK_TOL)).sum())
                q = pca.fit(x, 3, joint)
                cos = float((1 - (p.components * q.components).sum(-1).abs()).max())
                sub_ms, eigh_ms = interleaved([lambda: pca.fit(x, 3, joint, "subspace"), lambda: pca.fit(x, 3, joint)], args.rounds)
            mat = ops.covariance(x, None, joint)[1] if p.side == "covariance" else ops.gram(x)[1]
            n = mat.shape[-1]
            (av_ms,) = interleaved([lambda: ops.sym_topk(mat, 3, 0.0, 20)], args.rounds)  # 20 iterations, never done early
            (one_ms,) = interleaved([lambda: ops.sym_topk(mat, 3, 0.0, 1)], args.rounds)
            per_iter = (av_ms - one_ms) / 19
            print(json.dumps({"fit": name, "input": kind, "problems": int(mat.shape[0]), "rows": int(x.shape[1] * (P if joint else 1)), "d": d,
                              "side": p.side, "n": n, "subspace_ms": round(sub_ms, 3), "eigh_ms": round(eigh_ms, 3),
                              "eigh_over_subspace": round(eigh_ms / sub_ms, 2), "iters_max": int(p.iters.max()),
                              "resid_max": float(p.resid.max()), "fell_back_to_eigh": fell_back, "one_minus_cos_to_eigh": cos,
                              "ms_per_iteration_all_three_kernels": round(per_iter, 4),
                              "A_TB_per_s_if_the_iteration_were_A_V_alone": round(mat.numel() * 4 / per_iter / 1e9, 3)}), flush=True)
            del x, mat
            torch.cuda.empty_cache()


def binned_rows(args, ops, pca):
    for t in (196, 729):
        x = make_map("decay", 1, t, 13056, torch.bfloat16, t)
        p = pca.fit(x, 3, solver="subspace")
        (ms,) = interleaved([lambda: pca.fit(x, 3, solver="subspace")], args.rounds)
        g_ms, b_ms = interleaved([lambda: ops.gram(x), lambda: ops.pca_back_project(x, p.mean, p.scores.transpose(1, 2).contiguous(),
                                                                                  p.explained_variance.float())], args.rounds)
        print(json.dumps({"binned": f"{t} x 13056 bf16", "side": p.side, "fit_subspace_ms": round(ms, 3), "iters": int(p.iters.max()),
                          "resid": float(p.resid.max()), "mean_plus_gram_ms": round(g_ms, 4), "back_project_ms": round(b_ms, 4),
                          "map_read_TB_per_s_gram": round(x.numel() * 2 / g_ms / 1e9, 3)}), flush=True)


def e2e_rows(args, vdr):
    from oracle import vit_oracle as vo
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(vo.VitCfg(), seed=1, scale=0.02))
    for size, stride, B in ((224, 16, 16), (224, 8, 16), (512, 8, 1)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        x = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            e_ms, s_ms, x_ms = interleaved([lambda: model.pca_descriptors(x, facet="key"),
                                            lambda: model.pca_descriptor_maps(x, facet="key", solver="subspace"),
                                            lambda: model.extract_descriptors(x, facet="key")], args.rounds)
            row = {"e2e": "vit_base16 key facet", "size": size, "stride": stride, "grid": list(model.grid), "batch": B,
                   "pca_descriptors_eigh_ms": round(e_ms, 3), "pca_descriptors_subspace_ms": round(s_ms, 3),
                   "extract_descriptors_ms": round(x_ms, 3)}
            if model.grid[0] * model.grid[1] <= 4096:
                (b_ms,) = interleaved([lambda: model.pca_descriptor_maps(x, facet="key", bin=True, solver="subspace")], args.rounds)
                row["binned_subspace_ms"] = round(b_ms, 3)
        print(json.dumps(row), flush=True)


def iters_rows(vdr, pca):
    import time
    import pca_ref as pref
    from oracle import vit_oracle as vo

    def say(**kw):
        print(json.dumps(kw), flush=True)
    for name in pref.SK_CASES + ("pca_ref_colorize",):
        g, x = pref.load_golden(os.path.join(ROOT, "tests", "golden"), name)
        p = pca.fit(x.cuda(), 3, solver="subspace", max_iter=600)
        say(kind="golden", name=name, side=p.side, iters=p.iters.tolist(), resid=p.resid.tolist())
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(vo.VitCfg(), seed=1, scale=0.02))
    for size, stride, B in ((224, 16, 16), (224, 8, 16), (512, 8, 1)):
        model.set_input_size(size, size)
        model.set_patch_stride(stride)
        x = torch.rand(B, 3, size, size).to(torch.bfloat16).cuda()
        for binned in (False, True):
            if binned and size == 512:
                continue
            d = model.extract_descriptors(x[:4] if binned else x, facet="key", bin=binned)[:, 0].to(torch.bfloat16)
            for joint in ((False,) if binned else (False, True)):
                p = pca.fit(d, 3, joint=joint, solver="subspace", max_iter=600)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p = pca.fit(d, 3, joint=joint, solver="subspace", max_iter=int(2 * p.iters.max()))
                torch.cuda.synchronize()
                say(kind="model", size=size, stride=stride, shape=list(d.shape), binned=binned, joint=joint, side=p.side,
                    iters=p.iters.tolist(), resid_max=float(p.resid.max()), subspace_ms=(time.perf_counter() - t0) * 1e3)
            del d
    for P, t, d in ((4, 196, 768), (1, 3969, 768)):
        x = make_map("white", P, t, d, torch.bfloat16, t + d)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = pca.fit(x, 3, solver="subspace", max_iter=1500)
        say(kind="white noise", shape=[P, t, d], side=p.side, iters=p.iters.tolist(), resid=p.resid.tolist())


def tol_rows(ops):
    import numpy as np
    import pca_topk_ref as tref
    for n in (200, 768, 2048, 4096):
        for ratio in (0.5, 0.9):
            a, _, _ = tref.planted(n, tref.geometric(n, ratio), seed=n)
            ad = torch.from_numpy(a).unsqueeze(0).cuda()
            for k in (3, 8):
                floor = {m: float(ops.sym_topk(ad, k, 0.0, m)[3][0]) for m in (5, 10, 20, 40, 80)}
                val, vec, it, res = ops.sym_topk(ad, k)
                v64, l64 = vec[0].cpu().numpy().astype(np.float64), val[0].cpu().numpy().astype(np.float64)
                true = float(np.linalg.norm(a.astype(np.float64) @ v64.T - v64.T * l64, axis=0).max())
                print(json.dumps({"tol": "planted", "n": n, "ratio": ratio, "k": k, "resid_after_iters": floor,
                                  "default_iters": int(it[0]), "default_resid": float(res[0]), "float64_residual": true}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--e2e", type=int, default=1)
    ap.add_argument("--tol", type=int, default=1)
    ap.add_argument("--only", choices=("iters",), default=None, help="iters: the iteration counts alone")
    args = ap.parse_args()
    import vdr
    from vdr import ops, pca
    torch.cuda.set_device(0)
    print(json.dumps({"source_id": vdr.source_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                      "tol": ops.TOPK_TOL, "max_iter": ops.TOPK_MAX_ITER}), flush=True)
    if args.only == "iters":
        return iters_rows(vdr, pca)
    fit_rows(args, vdr, ops, pca)
    binned_rows(args, ops, pca)
    if args.e2e:
        e2e_rows(args, vdr)
    if args.tol:
        tol_rows(ops)
    iters_rows(vdr, pca)


if __name__ == "__main__":
    main()
