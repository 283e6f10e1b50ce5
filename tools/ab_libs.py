#!/usr/bin/env python3
"""Kernel-level A/B of two builds of libvdr.so in ONE process, interleaved rounds (guide rule 24): both libraries are
dlopen'ed side by side and the attention ops / vdr_op_linear_packed are called through ctypes on the same tensors.
   python tools/ab_libs.py path/to/libA.so[:variant] path/to/libB.so[:variant] [attention|gemm|descriptors|masks]
(":variant" = the tile variant handed to vdr_op_linear_packed by that side, e.g. the same library twice as lib.so:0 lib.so:31)
attention: first a bitwise pass (torch.equal of the two libraries' outputs) over the smallest shapes that reach every
instantiation of the fused attention kernels, then the timing; exit status 1 if any output differs.  For the spread of
the timing run a copy of library A against it (a second path: the same path is the same handle).
descriptors: the same two passes for the descriptor-analysis ops (nn_cosine, affinity_bits, local_correlation, the PCA ops, the
Gram side, k-means, mahalanobis): bitwise on the smallest shapes that reach every path (the shapes of the exact tests), every element of
every output compared; timed on the shapes of tools/correspondence_bench.py, spectral_bench.py (the affinity shapes),
local_correlation_bench.py, pca_bench.py, pca_topk_bench.py and kmeans_bench.py.
masks: the same two passes for the mask-plane ops (mask_stats, mask_binarize, connected_components, mask_clean in every mode,
distance_transform in every output combination, mask_box where both libraries export it): bitwise on the shapes of their exact
tests, int32 and uint8 planes included; timed on the shapes of tools/amg_bench.py, components_bench.py and edt_bench.py."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
from vdr import _lib  # noqa: E402

F32, BF16 = _lib.VDR_F32, _lib.VDR_BF16
GRAM_CHUNK = 256  # VDR_GRAM_CHUNK


def load(path):
    """the signatures of vdr/_lib.py on the library at `path`; one built before an entry point existed simply lacks it"""
    return _lib.bind(C.CDLL(path), skip_missing=True)


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


# ---- descriptor ops -------------------------------------------------------------------------------------------------
# A case is (name, run(lib, keep=None) -> outputs): run calls the ops and returns every output tensor.  keep is None (the bitwise
# pass): fresh outputs, floats prefilled with NaN, int32 with INT32_MIN, the scratch with 0xFF bytes; outputs that an op also reads
# (labels, centroids) start from the value the op's contract asks for instead.  keep is a list (the timing): the buffers are made
# on the first call, kept in it and shared by both libraries, and nothing is prefilled again.
_INT_FILL = -2 ** 31


class _Bufs:
    def __init__(self, keep):
        self.keep, self.i = keep, 0

    def get(self, make):
        if self.keep is None:
            return make()
        if self.i == len(self.keep):
            self.keep.append(make())
        self.i += 1
        return self.keep[self.i - 1]

    def out(self, *shape, dtype=torch.float32, value=None):
        if value is None:
            value = float("nan") if dtype.is_floating_point else _INT_FILL
        return self.get(lambda: torch.full(shape, value, device="cuda", dtype=dtype))

    def work(self, nbytes):
        return self.get(lambda: torch.full((nbytes,), 255, device="cuda", dtype=torch.uint8))


def _map(P, rows, d, ld, bf16, seed):
    """[P, rows, ld] with a channel offset (the centring has something to remove); the ld - d padding columns are NaN"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.full((P, rows, ld), float("nan"), device="cuda")
    x[..., :d] = torch.randn(P, rows, d, device="cuda", generator=gen) * 2 + torch.randn(d, device="cuda", generator=gen)
    return x.to(torch.bfloat16 if bf16 else torch.float32)


def nn_case(st, P, tx, ty, d, cols=True, pad=0):
    gen = torch.Generator(device="cuda").manual_seed(tx + ty + d)
    x = torch.randn(P, tx, d + pad, device="cuda", generator=gen).bfloat16()
    y = torch.randn(P, ty, d + pad, device="cuda", generator=gen).bfloat16()

    def run(lib, keep=None):
        o = _Bufs(keep)
        work = o.work(lib.vdr_nn_cosine_work_bytes(P, tx, ty))
        rs, ri = o.out(P, tx), o.out(P, tx, dtype=torch.int32)
        cs, ci = (o.out(P, ty), o.out(P, ty, dtype=torch.int32)) if cols else (None, None)
        assert lib.vdr_op_nn_cosine(x.data_ptr(), d + pad, tx * (d + pad), tx, y.data_ptr(), d + pad, ty * (d + pad), ty, P, d, work.data_ptr(),
                                    rs.data_ptr(), ri.data_ptr(), cs.data_ptr() if cols else None, ci.data_ptr() if cols else None, st) == 0
        return [rs, ri] + ([cs, ci] if cols else [])
    return f"nn_cosine P{P} tx{tx} ty{ty} d{d} cols{int(cols)}", run


def pca_case(st, P, imgs, t, d, bf16, ops=("mean", "cov", "proj"), pad=0):
    """col_mean -> covariance -> pca_project (k = 3, scaled) on `P` problems of `imgs` images; `ops` picks what is (re)run"""
    ld, R = d + pad, imgs * t
    x = _map(P * imgs, t, d, ld, bf16, t + d + imgs)
    comps = torch.randn(P, 3, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(d))
    mean0 = x[..., :d].float().reshape(P, R, d).mean(1).contiguous()  # the ops after col_mean read this one when col_mean is not run

    def run(lib, keep=None):
        a = (x.data_ptr(), BF16 if bf16 else F32, ld, t * ld, P, imgs, t, d)
        o = _Bufs(keep)
        work = o.work(lib.vdr_pca_work_bytes(P, imgs, t, d))
        outs, mean = [], mean0
        if "mean" in ops:
            mean = o.out(P, d)
            assert lib.vdr_op_col_mean(*a, work.data_ptr(), mean.data_ptr(), st) == 0
            outs.append(mean)
        if "cov" in ops and R >= 2:
            cov = o.out(P, d, d)
            assert lib.vdr_op_covariance(*a, mean.data_ptr(), work.data_ptr(), cov.data_ptr(), st) == 0
            outs.append(cov)
        if "proj" in ops:
            proj, mm = o.out(P, R, 3), o.out(P, 2)
            assert lib.vdr_op_pca_project(*a, mean.data_ptr(), comps.data_ptr(), 3, 1, work.data_ptr(), proj.data_ptr(), mm.data_ptr(), st) == 0
            outs += [proj, mm]
        return outs
    return f"pca {'+'.join(ops)} P{P} imgs{imgs} t{t} d{d} {'bf16' if bf16 else 'fp32'}", run


def gram_case(st, P, t, d, bf16, ops=("mean", "gram", "back"), pad=0):
    """col_mean_any -> gram -> pca_back_project (k = 3; the last component's value is 0: written as zeros)"""
    ld = d + pad
    x = _map(P, t, d, ld, bf16, t + d)
    gen = torch.Generator(device="cuda").manual_seed(t)
    u = torch.randn(P, 3, t, device="cuda", generator=gen)
    values = torch.tensor([[2.0, 1.0, 0.0]] * P, device="cuda")
    mean0 = x[..., :d].float().mean(1).contiguous()

    def run(lib, keep=None):
        a = (x.data_ptr(), BF16 if bf16 else F32, ld, t * ld, P, t, d)
        o = _Bufs(keep)
        work = o.work(lib.vdr_pca_topk_work_bytes(P, t, d, 8))
        outs, mean = [], mean0
        if "mean" in ops:
            mean = o.out(P, d)
            assert lib.vdr_op_col_mean_any(*a, work.data_ptr(), mean.data_ptr(), st) == 0
            outs.append(mean)
        if "gram" in ops:
            g = o.out(P, t, t)
            assert lib.vdr_op_gram(*a, mean.data_ptr(), work.data_ptr(), g.data_ptr(), st) == 0
            outs.append(g)
        if "back" in ops:
            comps = o.out(P, 3, d)
            assert lib.vdr_op_pca_back_project(*a, mean.data_ptr(), u.data_ptr(), values.data_ptr(), 3, work.data_ptr(), comps.data_ptr(), st) == 0
            outs.append(comps)
        return outs
    return f"gram {'+'.join(ops)} P{P} t{t} d{d} {'bf16' if bf16 else 'fp32'}", run


def kmeans_case(st, P, imgs, t, d, k, ops=("assign", "update")):
    """assign from labels = -1 (every row counts as changed), update from the centroids the assign read; the update alone runs on
    labels r % k"""
    R = imgs * t
    gen = torch.Generator(device="cuda").manual_seed(R + d + k)
    x = torch.randn(P, R, d, device="cuda", generator=gen).bfloat16()
    c0 = x[:, :k].float().contiguous()
    lab0 = (torch.arange(R, device="cuda", dtype=torch.int32) % k).repeat(P, 1).contiguous()

    def run(lib, keep=None):
        a = (x.data_ptr(), d, t * d, R * d, P, imgs, t, d, k)
        o = _Bufs(keep)
        work = o.work(lib.vdr_kmeans_work_bytes(P, imgs, t, d, k))
        outs, labels = [], lab0
        if "assign" in ops:
            labels = o.out(P, R, dtype=torch.int32, value=-1)
            md, inertia, changed = o.out(P, R), o.out(P), o.out(P, dtype=torch.int32)
            assert lib.vdr_op_kmeans_assign(*a, c0.data_ptr(), None, work.data_ptr(), labels.data_ptr(), md.data_ptr(), inertia.data_ptr(),
                                            changed.data_ptr(), st) == 0
            outs += [labels, md, inertia, changed]
        if "update" in ops:
            cent, counts = o.get(c0.clone), o.out(P, k, dtype=torch.int32)
            assert lib.vdr_op_kmeans_update(*a, labels.data_ptr(), None, work.data_ptr(), cent.data_ptr(), counts.data_ptr(), st) == 0
            outs += [cent, counts]
        return outs
    return f"kmeans {'+'.join(ops)} P{P} imgs{imgs} t{t} d{d} k{k}", run


def affinity_case(st, P, t, d, diag, pad=0, tau=0.05):
    """random rows: the cosines spread around 0 by 1 / sqrt(d), so tau = 0.05 sets a good share of the bits at every d; the
    padding columns of the rows are NaN"""
    ld = d + pad
    x = torch.full((P, t, ld), float("nan"), device="cuda")
    x[..., :d] = torch.randn(P, t, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(t + d))
    x = x.bfloat16()
    pitch = (t + 127) // 128 * 4

    def run(lib, keep=None):
        o = _Bufs(keep)
        work = o.work(lib.vdr_affinity_work_bytes(P, t))
        bits = o.out(P, t, pitch, dtype=torch.int32)
        assert lib.vdr_op_affinity_bits(x.data_ptr(), ld, t * ld, t, P, d, tau, diag, work.data_ptr(), bits.data_ptr(), pitch, st) == 0
        return [bits.view(torch.uint8)]
    return f"affinity P{P} t{t} d{d} diag{diag} pad{pad}", run


def local_case(st, P, grid, r, d, outs="cost+best", transposed=0, y_shared=False):
    """cost only, best only or both; y_shared: one Y map under every problem (problem stride 0)"""
    gh, gw = grid
    t, WW = gh * gw, (2 * r + 1) ** 2
    gen = torch.Generator(device="cuda").manual_seed(t + d + r)
    x = torch.randn(P, t, d, device="cuda", generator=gen).bfloat16()
    y = torch.randn(1 if y_shared else P, t, d, device="cuda", generator=gen).bfloat16()

    def run(lib, keep=None):
        o = _Bufs(keep)
        work = o.work(lib.vdr_local_correlation_work_bytes(P, gh, gw, r))
        cost = o.out(P, t, WW) if "cost" in outs else None
        bs, bi = (o.out(P, t), o.out(P, t, dtype=torch.int32)) if "best" in outs else (None, None)
        assert lib.vdr_op_local_correlation(x.data_ptr(), d, t * d, y.data_ptr(), d, 0 if y_shared else t * d, P, gh, gw, d, r, transposed,
                                            work.data_ptr(), cost.data_ptr() if cost is not None else None,
                                            bs.data_ptr() if bs is not None else None, bi.data_ptr() if bi is not None else None, st) == 0
        return [v for v in (cost, bs, bi) if v is not None]
    return f"local_corr P{P} {gh}x{gw} r{r} d{d} {outs}{' transposed' if transposed else ''}{' y_shared' if y_shared else ''}", run


def mahalanobis_case(st, P, t, d, k):
    gen = torch.Generator(device="cuda").manual_seed(t + d + k)
    x = torch.randn(P, t, d, device="cuda", generator=gen).bfloat16()
    mean = torch.randn(P, d, device="cuda", generator=gen)
    whiten = torch.randn(P, k, d, device="cuda", generator=gen) / d ** 0.5

    def run(lib, keep=None):
        d2 = _Bufs(keep).out(P, t)
        assert lib.vdr_op_mahalanobis(x.data_ptr(), d, t * d, t * d, P, 1, t, d, mean.data_ptr(), d, whiten.data_ptr(), k * d, k, d2.data_ptr(), st) == 0
        return [d2]
    return f"mahalanobis P{P} t{t} d{d} k{k}", run


def descriptors_equal(libs, st):
    """the shapes of the exact tests (tests/test_nn_cosine_gpu.py, test_affinity_gpu.py, test_local_correlation_gpu.py, test_pca_gpu.py,
    test_pca_topk_gpu.py, test_kmeans_gpu.py)"""
    cases = [nn_case(st, 2, tx, ty, d, cols, pad=8) for (tx, ty) in ((1, 1), (127, 129), (130, 257)) for d in (32, 96, 448) for cols in (True, False)]
    cases += [nn_case(st, 520, 17, 19, 32)]  # more work items than the split aims for: one split
    cases += [affinity_case(st, 2, t, d, diag) for t in (1, 33, 129, 300) for d in (32, 96, 448) for diag in (0, 1)]
    cases += [affinity_case(st, 2, 129, 96, 1, pad=32), affinity_case(st, 300, 130, 96, 1)]  # padded rows; 600 items: one run
    cases += [local_case(st, 2, grid, r, d, outs) for grid in ((1, 1), (5, 7), (9, 17), (17, 33)) for r in (1, 8) for d in (32, 96)
              for outs in ("cost", "best", "cost+best")]
    cases += [local_case(st, 2, (9, 17), 3, 96, transposed=1), local_case(st, 3, (9, 17), 3, 96, y_shared=True)]
    cases += [mahalanobis_case(st, 2, t, 96, k) for t in (129, 300) for k in (1, 130)]
    cases += [pca_case(st, 2, imgs, t, d, bf16, pad=32) for t in (2, 16, 17, 1025, 2049) for d in (32, 160, 288) for bf16 in (True, False)
              for imgs in (1, 2)]
    cases += [gram_case(st, 2, t, d, bf16, pad=32) for t in (17, 129, 300) for d in (96, GRAM_CHUNK + 32) for bf16 in (True, False)]
    cases += [kmeans_case(st, 2, 1, R, d, k) for R in (1, 129, 300) for k in (1, 127, 130) if k <= R for d in (96, 416)]
    return cases_equal(libs, cases)


def cases_equal(libs, cases, u8_fill=None):
    """every element of every output of every case, library A against library B; u8_fill: the value no uint8 output may keep"""
    def undefined(t):
        if t.dtype == torch.uint8:  # (without u8_fill: the affinity words as bytes -- in a bit field every pattern is a value, the fill included)
            return 0 if u8_fill is None else int((t == u8_fill).sum())
        return int((torch.isnan(t) if t.dtype.is_floating_point else t == _INT_FILL).sum())
    bad = 0
    for name, run in cases:
        outs = [run(lib) for lib in libs]
        torch.cuda.synchronize()
        notes = []  # per output that fails: its index, elements left undefined by A / B, elements whose bits differ
        for i, (a, b) in enumerate(zip(*outs)):
            undef = [undefined(t) for t in (a, b)]
            diff = int((a != b).sum()) if a.dtype == torch.uint8 else int((a.view(torch.int32) != b.view(torch.int32)).sum())
            if undef[0] or undef[1] or diff:
                notes.append(f"out{i} undefined {undef[0]}/{undef[1]} differ {diff} of {a.numel()}")
        same = len(outs[0]) == len(outs[1]) and not notes
        bad += not same
        print(f"equal {name:52s}: {same}" + "".join("  [" + n + "]" for n in notes), flush=True)
    print(f"bitwise pass: {len(cases)} cases, {bad} differ", flush=True)
    return bad


def descriptors_timed(st):
    timed = [nn_case(st, P, t, t, d) for (P, t, d) in ((64, 196, 768), (64, 196, 13056), (32, 729, 13056), (1, 3969, 13056), (8, 3969, 13056))]
    timed += [affinity_case(st, P, t, d, 1, tau=0.2) for (P, t, d) in ((64, 196, 768), (32, 729, 768), (1, 3969, 768), (1, 3969, 13056), (8, 3969, 768))]
    timed += [local_case(st, P, grid, r, d) for (P, grid, d, r) in ((64, (14, 14), 768, 2), (32, (27, 27), 768, 4), (1, (63, 63), 768, 4),
                                                                    (8, (63, 63), 768, 4), (1, (63, 63), 768, 8), (8, (63, 63), 768, 8),
                                                                    (1, (63, 63), 13056, 4))]
    timed += [mahalanobis_case(st, 8, 3969, 768, 100)]
    for (P, t, d, bf16) in ((64, 196, 768, True), (16, 729, 768, True), (16, 4096, 256, False), (1, 3969, 768, True)):
        for joint in ((False, True) if P > 1 else (False,)):
            timed += [pca_case(st, 1 if joint else P, P if joint else 1, t, d, bf16, (op,)) for op in ("mean", "cov", "proj")]
    timed += [gram_case(st, 1, t, 13056, True, (op,)) for t in (196, 729) for op in ("mean", "gram", "back")]
    for (P, imgs, t, d, k) in ((1, 8, 196, 768, 10), (1, 8, 729, 768, 10), (8, 1, 196, 13056, 10), (1, 1, 150, 26112, 10)):
        timed += [kmeans_case(st, P, imgs, t, d, k, (op,)) for op in ("assign", "update")]
    return timed


# ---- mask-plane ops ---------------------------------------------------------------------------------------------------
# Every output is an integer (mask_box: floats from integers by a fixed chain), so "equal" is the whole requirement.  uint8 outputs
# are prefilled with _U8_FILL, which no op writes (they write 0 / 1).
_U8_FILL = 255


def _blobs(P, H, W, seed):
    """uint8 [P, H, W]: smooth blobs with holes and specks (a coarse random field up-sampled, a little salt on top)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((P, 1, max(H // 16, 1) + 1, max(W // 16, 1) + 1), generator=g)
    m = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)[:, 0] > 0.1
    return (m ^ (torch.rand((P, H, W), generator=g) < 0.02)).to(torch.uint8).cuda()


def logits_case(st, H, W, oh, ow, P, tokens=None):
    """mask_stats and mask_binarize on [P, 4, H, W] logits: one token in place, tokens 1 .. 3 in place (groups), or dense"""
    lg = (torch.randn((P, 4, H, W), generator=torch.Generator().manual_seed(H + W + oh)) * 3).cuda()
    if tokens is None:
        a = (lg.data_ptr(), H * W, 4 * P, 0, 4 * P)
    elif tokens == 1:
        a = (lg[:, 2].data_ptr(), H * W, 1, 4 * H * W, P)
    else:
        a = (lg[:, 1:].data_ptr(), H * W, 3, 4 * H * W, 3 * P)
    n = a[4]

    def run(lib, keep=None):
        o = _Bufs(keep)
        work = o.work(lib.vdr_mask_stats_workspace_bytes(n, H, W, oh, ow))
        counts, box = o.out(n, 3, dtype=torch.int32), o.out(n, 4, dtype=torch.int32)
        assert lib.vdr_op_mask_stats(*a, H, W, oh, ow, 0.25, 0.75, work.data_ptr(), work.numel(), counts.data_ptr(), box.data_ptr(), st) == 0
        plane = o.out(n, oh, ow, dtype=torch.uint8, value=_U8_FILL)
        assert lib.vdr_op_mask_binarize(*a, H, W, oh, ow, 0.25, work.data_ptr(), work.numel(), plane.data_ptr(), st) == 0
        return [counts, box, plane]
    return f"mask_stats+binarize {H}x{W}->{oh}x{ow} P{n} {'dense' if tokens is None else 'token' if tokens == 1 else 'groups'}", run


def components_case(st, P, H, W, ops=("label", 0, 1, 2, 3, 4, 5)):
    """connected_components (conn 8, value 1) and mask_clean in every mode (0: the copy; 1 holes, 2 islands, 4 largest)"""
    m = _blobs(P, H, W, H + 3 * W)

    def run(lib, keep=None):
        o = _Bufs(keep)
        outs = []
        if "label" in ops:
            work = o.work(lib.vdr_connected_components_workspace_bytes(P, H, W))
            root, area, count = o.out(P, H, W, dtype=torch.int32), o.out(P, H, W, dtype=torch.int32), o.out(P, dtype=torch.int32)
            assert lib.vdr_op_connected_components(m.data_ptr(), P, H, W, 8, 1, work.data_ptr(), work.numel(), root.data_ptr(), area.data_ptr(),
                                                   count.data_ptr(), st) == 0
            outs += [root, area, count]
        work = o.work(lib.vdr_mask_clean_workspace_bytes(P, H, W))
        for mode in (v for v in ops if v != "label"):
            out = o.out(P, H, W, dtype=torch.uint8, value=_U8_FILL)
            changed, stats = o.out(P, dtype=torch.int32), o.out(P, 5, dtype=torch.int32)
            assert lib.vdr_op_mask_clean(m.data_ptr(), P, H, W, 9, 4 if mode & 1 else 8, mode, work.data_ptr(), work.numel(), out.data_ptr(),
                                         changed.data_ptr(), stats.data_ptr(), st) == 0
            outs += [out, changed, stats]
        return outs
    return f"components {'+'.join(str(v) for v in ops)} P{P} {H}x{W}", run


EDT_OUTPUTS = ("d2", "nearest", "peak", "within", "d2+nearest+peak", "within+peak", "d2+peak")


def edt_case(st, P, H, W, outputs, value=1, outside=0):
    """distance_transform with one combination of its outputs (the peak alone included)"""
    m = _blobs(P, H, W, 5 * H + W)
    if P > 1:
        m[0] = 0  # a plane with nothing selected (value 1): peak (0, -1)
    want = outputs.split("+")

    def run(lib, keep=None):
        o = _Bufs(keep)
        work = o.work(lib.vdr_distance_transform_workspace_bytes(P, H, W))
        d2 = o.out(P, H, W, dtype=torch.int32) if "d2" in want else None
        nearest = o.out(P, H, W, dtype=torch.int32) if "nearest" in want else None
        peak = o.out(P, 2, dtype=torch.int32) if "peak" in want else None
        within = o.out(P, H, W, dtype=torch.uint8, value=_U8_FILL) if "within" in want else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        assert lib.vdr_op_distance_transform(m.data_ptr(), P, H, W, value, outside, 10, work.data_ptr(), work.numel(), ptr(d2), ptr(nearest), ptr(peak),
                                             ptr(within), st) == 0
        return [t for t in (d2, nearest, peak, within) if t is not None]
    return f"edt {outputs} P{P} {H}x{W} v{value} o{outside}", run


def box_case(st, P, H, W):
    """mask_box: random planes, one empty plane (prev comes back), one plane whose only pixel is the last"""
    lg = torch.randn((P, H, W), generator=torch.Generator().manual_seed(H * W)).cuda() - 1.5
    lg[0] = -1.0
    if P > 1:
        lg[1] = -1.0
        lg[1, H - 1, W - 1] = 1.0
    prev = torch.rand((P, 4), generator=torch.Generator().manual_seed(P)).cuda() * 100

    def run(lib, keep=None):
        o = _Bufs(keep)
        boxes, area = o.out(P, 4), o.out(P, dtype=torch.int32)
        assert lib.vdr_op_mask_box(lg.data_ptr(), H * W, prev.data_ptr(), boxes.data_ptr(), area.data_ptr(), P, H, W, 1024, 2.5, 0.0, st) == 0
        return [boxes, area]
    return f"mask_box P{P} {H}x{W}", run


def masks_equal(libs, st):
    """the shapes of the exact tests (tests/test_amg_gpu.py, test_components_gpu.py, test_edt_gpu.py, the mask_box cases of
    test_sam_prompts_gpu.py), the 65-chunk plane of mask_clean and the 128-band plane of mask_stats included"""
    cases = [logits_case(st, H, W, oh, ow, P, tok) for (H, W, oh, ow, P) in ((1, 1, 3, 5, 3), (8, 8, 32, 32, 130), (12, 20, 50, 75, 130), (17, 3, 9, 2, 3),
                                                                             (64, 64, 256, 256, 3), (256, 256, 1024, 1024, 1), (5, 7, 4096, 33, 3))
             for tok in (None, 1, 3)]
    planes = ((1, 1), (1, 129), (2, 64), (63, 65), (64, 64), (65, 129), (129, 129), (129, 257), (300, 517), (513, 513))
    cases += [components_case(st, 3, H, W) for (H, W) in planes]
    cases += [edt_case(st, 3, H, W, outputs) for (H, W) in planes + ((1, 4096), (4096, 1)) for outputs in EDT_OUTPUTS]
    cases += [edt_case(st, 3, 300, 517, "d2+peak", value, outside) for value in (0, 1) for outside in (0, 1)]
    if all(hasattr(lib, "vdr_op_mask_box") for lib in libs):
        cases += [box_case(st, 3, H, W) for (H, W) in ((1, 1), (5, 7), (16, 16), (33, 7), (256, 256), (64, 1028))]
    return cases_equal(libs, cases, u8_fill=_U8_FILL)


def masks_timed(libs, st):
    """the shapes of tools/amg_bench.py, components_bench.py and edt_bench.py; mask_box on 256 x 256 planes"""
    timed = [logits_case(st, 256, 256, 1024, 1024, 64, 3), logits_case(st, 256, 256, 1024, 1024, 1, 1)]
    for P, side in ((1, 1024), (64, 1024), (192, 256)):
        timed += [components_case(st, P, side, side, ("label",)), components_case(st, P, side, side, (3,)), components_case(st, P, side, side, (4,))]
        timed += [edt_case(st, P, side, side, "d2"), edt_case(st, P, side, side, "peak"), edt_case(st, P, side, side, "d2+nearest+peak")]
    if all(hasattr(lib, "vdr_op_mask_box") for lib in libs):
        timed += [box_case(st, 1, 256, 256), box_case(st, 64, 256, 256)]
    return timed


def main():
    specs =[a.split(":") for a in sys.argv[1:3]]
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
    elif what in ("descriptors", "masks"):
        bad = descriptors_equal(libs, st) if what == "descriptors" else masks_equal(libs, st)
        for name, run in (descriptors_timed(st) if what == "descriptors" else masks_timed(libs, st)):
            keep = []
            for li, lib in enumerate(libs):
                cases.append((f"{name} lib{'AB'[li]}", lambda lib=lib, run=run, keep=keep: 0 if run(lib, keep) is not None else 1))
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
