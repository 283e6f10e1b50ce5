#!/usr/bin/env python3
"""Kernel-level A/B of two builds of libvdr.so in ONE process, interleaved rounds (guide rule 24): both libraries are
dlopen'ed side by side and the attention ops / vdr_op_linear_packed are called through ctypes on the same tensors.
   python tools/ab_libs.py path/to/libA.so[:variant] path/to/libB.so[:variant] [attention|gemm]
(":variant" = the tile variant handed to vdr_op_linear_packed by that side, e.g. the same library twice as lib.so:0 lib.so:31)
attention: first a bitwise pass (torch.equal of the two libraries' outputs) over the smallest shapes that reach every
instantiation of the fused attention kernels, then the timing; exit status 1 if any output differs.  For the spread of
the timing run a copy of library A against it (a second path: the same path is the same handle)."""
import ctypes as C
import sys

import torch

_P, _I = C.c_void_p, C.c_int


def load(path):
    lib = C.CDLL(path)
    lib.vdr_op_attention.argtypes = [_P, _P, _I, _I, _I, _I, _P]
    lib.vdr_op_attention_hd.argtypes = [_P, _P, _I, _I, _I, _I, _I, _P]
    lib.vdr_op_attention_varlen.argtypes = [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P]
    lib.vdr_op_attention_relpos.argtypes = [_P, _P, _P, _P, _P, _I, _I, _I, _P]
    lib.vdr_op_linear_packed.argtypes = [_P] * 6 + [C.c_int64, _I, _I, _I, _I, _P]
    lib.vdr_op_pack_linear_weight.argtypes = [_P, _I, _I, _P, _P]
    return lib


def attn_case(st, B, N, H, variant=0, dh=64, lens=None):
    """-> (name, call(lib, out) -> status, out shape, rows of the output that are defined)"""
    qkv = torch.randn(B * N, 3 * H * dh, device="cuda").bfloat16()
    name = f"attention dh{dh} B{B} N{N} H{H} v{variant}"
    if lens is not None:
        ln = torch.tensor([lens[b % len(lens)] for b in range(B)], device="cuda", dtype=torch.int32)
        valid = (torch.arange(N, device="cuda")[None, :] < ln[:, None]).reshape(-1)
        return (name + f" lens{lens}", lambda lib, out: lib.vdr_op_attention_varlen(
            qkv.data_ptr(), out.data_ptr(), B, N, H, dh, ln.data_ptr(), 0, variant, st), (B * N, H * dh), valid)
    if dh != 64:
        return name, lambda lib, out: lib.vdr_op_attention_hd(qkv.data_ptr(), out.data_ptr(), B, N, H, dh, variant, st), (B * N, H * dh), None
    return name, lambda lib, out: lib.vdr_op_attention(qkv.data_ptr(), out.data_ptr(), B, N, H, variant, st), (B * N, H * dh), None


def relpos_case(st, B, S, H):
    qkv = torch.randn(B * S * S, 3 * H * 64, device="cuda").bfloat16()
    rh, rw = (torch.randn(2 * S - 1, 64, device="cuda") * 0.2 for _ in range(2))
    npad = 2 * ((2 * S - 1 + 31) // 32 * 32)
    rel = torch.empty(B * S * S * H * npad + npad * 32, device="cuda")
    return (f"relpos S{S} B{B} H{H}", lambda lib, out: lib.vdr_op_attention_relpos(
        qkv.data_ptr(), rh.data_ptr(), rw.data_ptr(), rel.data_ptr(), out.data_ptr(), B, S, H, st), (B * S * S, H * 64), None)


def attention_equal(libs, st):
    """the smallest shapes that reach each instantiation: NT 2 / 4 / 7 / 9, chunked, every variant, the loader-wave choice
    (516 items), per-sequence lengths, head dims 32 / 96 / 128, the rel-pos window sizes, both run-time-grid forms"""
    cases = [attn_case(st, 2, n, 3) for n in (5, 100, 197, 257, 300)]
    cases += [attn_case(st, 2, 100, 3, 2)] + [attn_case(st, 2, 197, 3, v) for v in (1, 2, 3, 4)] + [attn_case(st, 43, 197, 12)]
    cases += [attn_case(st, 5, 160, 3, lens=(1, 17, 64, 129, 160))]
    for dh in (32, 96, 128):
        for n in (33, 197):
            cases += [attn_case(st, 2, n, 2, dh=dh), attn_case(st, 3, n, 2, dh=dh, lens=(1, 17, 33))]
    cases += [relpos_case(st, 3, s, 2) for s in (4, 7, 10, 14)] + [relpos_case(st, 1, s, 2) for s in (64, 9, 33, 48, 57)]
    bad = 0
    for name, call, shape, valid in cases:
        outs = []
        for lib in libs:
            out = torch.full(shape, float("nan"), device="cuda", dtype=torch.bfloat16)
            assert call(lib, out) == 0, name
            torch.cuda.synchronize()
            outs.append(out if valid is None else out[valid])
        same = torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and not torch.isnan(outs[0]).any().item()
        bad += not same
        print(f"equal {name:52s}: {same}", flush=True)
    print(f"bitwise pass: {len(cases)} cases, {bad} differ", flush=True)
    return bad


def main():
    specs = [a.split(":") for a in sys.argv[1:3]]
    libs = [load(sp[0]) for sp in specs]
    variants = [int(sp[1]) if len(sp) > 1 else 0 for sp in specs]
    what = sys.argv[3] if len(sys.argv) > 3 else "attention"
    st = torch.cuda.current_stream().cuda_stream
    cases, bad = [], 0
    if what == "attention":
        bad = attention_equal(libs, st)
        timed = [attn_case(st, B, N, H) for (B, N, H) in ((256, 197, 12), (64, 577, 16), (32, 257, 24))]
        timed += [attn_case(st, 130, 197, 4, dh=96), relpos_case(st, 25 * 16, 14, 12), relpos_case(st, 16, 64, 12),
                  relpos_case(st, 16, 32, 12), relpos_case(st, 16, 48, 12)]
        for name, call, shape, _ in timed:
            out = torch.empty(shape, device="cuda", dtype=torch.bfloat16)
            for li, lib in enumerate(libs):
                cases.append((f"{name} lib{'AB'[li]}", lambda lib=lib, call=call, out=out: call(lib, out)))
    else:
        M = 50432
        for name, N, K, epi in (("qkv", 2304, 768, 0), ("fc1", 3072, 768, 1)):
            x = torch.randn(M, K, device="cuda").bfloat16()
            W = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
            Wp = torch.empty_like(W)
            libs[0].vdr_op_pack_linear_weight(W.data_ptr(), N, K, Wp.data_ptr(), st)
            b = torch.randn(N, device="cuda")
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            for li, lib in enumerate(libs):
                cases.append((f"gemm {name} lib{'AB'[li]}", lambda lib=lib, x=x, Wp=Wp, b=b, out=out, N=N, K=K, epi=epi, v=variants[li]:
                              lib.vdr_op_linear_packed(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), None, None, out.data_ptr(), M, N, K, epi, v, st)))
    for _, f in cases:
        assert f() == 0
    torch.cuda.synchronize()
    ts = [[] for _ in cases]
    for rnd in range(22):
        # the two libraries of a pair run back to back on the same tensors: alternate who goes first, or the second one
        # inherits warm caches every time (identical kernels differed by 3-7 % with a fixed order)
        order = list(range(len(cases)))
        if rnd & 1:
            order = [i ^ 1 for i in order]
        ev = {}
        for i in order:
            f = cases[i][1]
            a, b2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); f(); b2.record(); ev[i] = (a, b2)
        torch.cuda.synchronize()
        for i, (a, b2) in ev.items():
            ts[i].append(a.elapsed_time(b2) / 2)
    med = []
    for (n, _), t in zip(cases, ts):
        t = sorted(t)
        med.append(t[len(t) // 2])
        print(f"{n:44s}: median {t[len(t) // 2] * 1e3:8.1f} us  min {t[0] * 1e3:8.1f}", flush=True)
    for i in range(0, len(cases), 2):
        print(f"{cases[i][0][:-5]:40s}: median B - A {(med[i + 1] - med[i]) * 1e3:+7.1f} us ({(med[i + 1] / med[i] - 1) * 100:+.2f} %)", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
