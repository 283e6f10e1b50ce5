"""GPU: the workspace contract of every forward (include/vdr.h at vdr_workspace_bytes).

  1. A forward touches nothing outside [workspace, workspace + vdr_workspace_bytes).
  2. Its outputs do not depend on what the workspace held on entry.
  3. With fewer bytes than that it returns VDR_ERR_WORKSPACE and has written nothing.

carve() (csrc/vdr_api.hip) cuts the workspace into a dozen buffers whose sizes carry hand-written slack (row counts padded
to 256 + 256, + 4096 on the col buffers, + 256 on rel), other code borrows them for second uses (POOLED in the fc1 buffer,
im2col in u), and kernels read rows they do not own (a ragged last 8-phase tile, the MX scale pairs (r, r + 32), padded LN
partial slots).  Engine hands over a torch.empty, i.e. whatever the allocator last held, so a read-before-write is a rare
flaky gate.  Here the workspace is the middle of one larger allocation (tests/memguard.py): exactly `need` bytes, 256-byte
aligned, between two canary guards of 4 MiB -- at least 512 rows of the widest row of any case, so a miscount of one whole
padding step of carve() lands inside memory this test owns -- and is prefilled with zeros, with 0xFF bytes (NaN as bf16,
fp32, e4m3 and e8m0 alike) and with bf16 1000.0.  The Engine instance's _workspace is overridden, so every entry point is
reached through its existing wrapper.

Cases: the launch ledger's (the smallest shape that reaches each branch of the forward, and ViT-B width at batch 100 for
the 8-phase GEMMs' ragged last row tile), plus facets with log-binning, a patch stride of p / 2, a non-native non-square
input size, a CLIP and a SigLIP tower, a resized SAM encoder and a varlen token forward that returns every row.

A failure here is a finding in the library: localise it with workspace_fill_range (fill only part of the body, halve
until one buffer of carve() remains) -- no debugger needed.
"""
import ctypes as C
import os

import pytest
import torch

import clip_ref as cr
import forward_cases as fc
import handle_configs as hc
import memguard as mg
from handle_configs import P16, POSTLN, SAM
from oracle import sam_oracle as so
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

GUARD = 4 << 20
VDR_ERR_WORKSPACE = -5
FILL_ORDER = ("zeros", "ones", "bf16_1000")


class Workspaces:
    """Overrides engine._workspace: every call gets a fresh guarded body of exactly `need - short` bytes, prefilled with
    pattern `fill` over bytes [lo, hi) (fractions of the body; the rest zeros), or left all canary (fill=None)."""

    def __init__(self, engine):
        self.e, self.fill, self.lo, self.hi, self.short, self.handed = engine, "zeros", 0.0, 1.0, 0, []
        c = engine.cfg
        assert GUARD >= 512 * max(3 * c.dim, c.mlp_hidden) * 2, "guard below 512 rows of the widest row"
        engine._workspace = self._workspace

    def _workspace(self, batch, seq=0):
        from vdr import _lib as L
        need = C.c_size_t()
        L.check(self.e.lib.vdr_workspace_bytes(self.e.h, batch, seq, C.byref(need)), self.e.h)
        whole, body = mg.guarded(need.value - self.short, GUARD)
        assert body.numel() == need.value - self.short and body.data_ptr() % 256 == 0
        if self.fill is not None:
            n = body.numel()
            lo, hi = int(self.lo * n) & ~255, n if self.hi >= 1.0 else int(self.hi * n) & ~255
            if (lo, hi) != (0, n):
                mg.fill(body, "zeros")
            mg.fill(body, self.fill, lo, hi)
        self.handed.append((whole, body))
        return body

    def check_guards(self, what):
        torch.cuda.synchronize()
        assert self.handed, f"{what}: the call asked for no workspace"
        for whole, body in self.handed:
            front, back = mg.guard_damage(whole, GUARD)
            assert (front, back) == (None, None), (f"{what}: wrote outside the workspace of {body.numel()} bytes: nearest damaged "
                                                   f"byte in front {front}, behind {back} (offsets from its start)")
        self.handed = []


# ---- cases the ledger does not have -----------------------------------------------------------------------------------------
def _p16(**kw):
    return hc.engine(P16, vo.make_weights(P16, seed=3, scale=0.05), **kw)


def _facets():
    import vdr
    e = _p16()
    x = vo.make_images(P16, 3, seed=4).cuda()

    def run():
        f, feats, maps = e.forward_descriptors(x, [vdr.FacetOut(1, "key", hierarchy=2), vdr.FacetOut(2, "token", all_rows=True),
                                                   vdr.FacetOut(0, "value", hierarchy=1, dtype=torch.bfloat16)],
                                               [vdr.LayerOut(1, vdr.OUT_CLS)], [vdr.AttnMap(1, q_rows=1)])
        return list(f) + list(feats) + list(maps)
    return e, run


def _half_stride():
    import vdr
    e = _p16()
    e.set_patch_stride(P16.patch // 2)  # 7 x 7 overlapping patches: the col buffer grows
    x = vo.make_images(P16, 3, seed=4).cuda()
    return e, lambda: [e.forward(x, vdr.OUT_DENSE), e.forward(x, vdr.OUT_CLS)]


def _other_size():
    import vdr
    e = _p16()
    e.set_input_size(96, 48)  # native 64 x 64
    x = torch.rand(3, 3, 96, 48, generator=torch.Generator().manual_seed(5)).cuda()
    return e, lambda: [e.forward(x, vdr.OUT_TOKENS), e.forward(x, vdr.OUT_CLS)]


def _tower(family):
    def make():
        g, cfg, w, model = cr.tiny_model(os.path.join(hc.HERE, "golden"), family)
        x = vo.make_images(cfg, 3, seed=8).cuda()
        return model.engine, lambda: [model.get_image_features(x)]
    return make


def _sam_resized():
    import vdr
    cs = hc.sized_sam(SAM, 112)  # native 160: a 7 x 7 grid, ragged 4 x 4 windows, resampled position tables
    e = hc.sam_engine(cs, so.make_weights(SAM, seed=21, scale=0.05))
    x = so.make_images(cs, 2, seed=22).cuda()
    return e, lambda: [e.forward(x, vdr.OUT_ENCODER)]


VARLEN = [5, 1, 17, 9]


def _postln_varlen_tokens():
    import vdr
    e = hc.engine(POSTLN, vo.make_weights(POSTLN, seed=13, scale=0.05))
    x = vo.make_tokens(4, 17, POSTLN.dim, seed=14).cuda()
    c = 1 if POSTLN.has_cls else 0

    def run():  # rows past a sequence's length are undefined (vdr.h): the defined rows only
        t = e.forward_tokens(x, vdr.OUT_TOKENS, lengths=VARLEN)
        d = e.forward_tokens(x, vdr.OUT_DENSE, lengths=VARLEN)
        return [t[b, :n + c] for b, n in enumerate(VARLEN)] + [d[b, :n] for b, n in enumerate(VARLEN)]
    return e, run


EXTRA = {"facets-binned": _facets, "patch_stride-half": _half_stride, "input_size-96x48": _other_size, "clip-tower": _tower("clip"),
         "siglip-tower": _tower("siglip"), "sam-resized-112": _sam_resized, "postln-varlen-all_rows": _postln_varlen_tokens}
CASES = list(fc.CASE_IDS) + list(EXTRA)
TWO_STREAMS = [c for c in fc.CASE_IDS if "mb2_streams2" in c]


def _maker(case):
    return EXTRA[case] if case in EXTRA else fc.cases()[case]


def _snapshot(outs):
    torch.cuda.synchronize()
    return [t.clone() for t in outs]


def _same_bits(got, ref, what):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if not torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)):
            n = int((a != b).sum() + (a.isnan() != b.isnan()).sum())
            raise AssertionError(f"{what}: output {k} {tuple(a.shape)} differs in {n} elements from the untouched engine's")


def _reference(case):
    """the outputs of the same call on an untouched engine of the same config (its own torch.empty workspace)"""
    e, run = _maker(case)()
    ref = _snapshot(run())
    e.close()
    return ref


@pytest.mark.parametrize("case", CASES)
def test_forward_stays_inside_its_workspace_and_ignores_its_contents(case):
    import vdr
    ref = _reference(case)
    e, run = _maker(case)()
    ws = Workspaces(e)
    for fill in FILL_ORDER:
        ws.fill = fill
        got = _snapshot(run())
        ws.check_guards(f"{case} fill {fill}")
        _same_bits(got, ref, f"{case} fill {fill}")
        if fill == "ones":
            for k, t in enumerate(got):
                assert torch.isfinite(t.float()).all(), f"{case}: output {k} not finite with a NaN-filled workspace"
    # 256 bytes short: refused, and neither the body nor the guards were written
    ws.fill, ws.short = None, 256
    with pytest.raises(vdr.VdrError) as err:
        run()
    assert err.value.code == VDR_ERR_WORKSPACE, err.value
    torch.cuda.synchronize()
    assert ws.handed
    for whole, _ in ws.handed:
        assert bool((whole == mg.CANARY).all()), f"{case}: a refused call wrote to its workspace"


@pytest.mark.parametrize("fill", ["ones", "bf16_1000"])
@pytest.mark.parametrize("case", TWO_STREAMS)
def test_second_stream_slice_alone(case, fill):
    """Micro-batches on two streams run in two halves of the workspace: the pattern in the second stream's slice only (the
    first zeros), then in the first only."""
    ref = _reference(case)
    e, run = _maker(case)()
    ws = Workspaces(e)
    ws.fill = fill
    for lo, hi in ((0.5, 1.0), (0.0, 0.5)):
        ws.lo, ws.hi = lo, hi
        got = _snapshot(run())
        ws.check_guards(f"{case} fill {fill} in [{lo}, {hi})")
        _same_bits(got, ref, f"{case} fill {fill} in [{lo}, {hi})")


def _canary(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * dtype.itemsize,), mg.CANARY, dtype=torch.uint8, device="cuda").view(dtype).view(shape)


def test_short_workspace_refused_by_every_entry_point_outputs_untouched():
    """vdr_forward, _layers, _attn_maps, _facets, _tokens and _tokens_varlen with need - 256 bytes: VDR_ERR_WORKSPACE; the
    canary-filled caller-owned outputs, the workspace body and its guards keep every byte."""
    import vdr
    from vdr import _lib as L
    e = _p16()
    ws = Workspaces(e)
    ws.fill, ws.short = None, 256
    B, D, N, n, H = 3, P16.dim, e.n_tokens, e.n_patches, P16.heads
    x = vo.make_images(P16, B, seed=4).cuda()
    outs = {k: _canary(s, torch.float32) for k, s in dict(cls=(B, D), tokens=(B, N, D), map=(B, H, 1, N), facet=(B, n, D)).items()}
    lo = lambda: vdr.LayerOut(1, vdr.OUT_CLS, out=outs["cls"])  # noqa: E731
    calls = {
        "vdr_forward": lambda: e.forward_into(x, outs["tokens"], vdr.OUT_TOKENS),
        "vdr_forward_layers": lambda: e.forward_layers(x, [lo(), vdr.LayerOut(2, vdr.OUT_TOKENS, out=outs["tokens"])]),
        "vdr_forward_attn_maps": lambda: e.forward_attn_maps(x, [vdr.AttnMap(1, 1, out=outs["map"])], [lo()]),
        "vdr_forward_facets": lambda: e.forward_descriptors(x, [vdr.FacetOut(1, "key", out=outs["facet"])], [lo()],
                                                            [vdr.AttnMap(1, 1, out=outs["map"])]),
    }
    for name, call in calls.items():
        with pytest.raises(vdr.VdrError) as err:
            call()
        assert err.value.code == VDR_ERR_WORKSPACE, (name, err.value)
    # the token entry points: Engine.forward_tokens allocates its output itself, so the C calls are made here
    t = hc.engine(POSTLN, vo.make_weights(POSTLN, seed=13, scale=0.05))
    tws = Workspaces(t)
    tws.fill, tws.short = None, 256
    Bt, S, Dt = 4, 17, POSTLN.dim
    tok = vo.make_tokens(Bt, S, Dt, seed=14).float().cuda().contiguous()
    tout = _canary((Bt, Dt), torch.float32)
    lens = torch.tensor(VARLEN, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for varlen in (False, True):
        body = tws._workspace(Bt, S)
        if varlen:
            rc = t.lib.vdr_forward_tokens_varlen(t.h, tok.data_ptr(), L.VDR_F32, Bt, S, lens.data_ptr(), tout.data_ptr(), vdr.OUT_CLS,
                                                 L.VDR_F32, body.data_ptr(), body.numel(), stream)
        else:
            rc = t.lib.vdr_forward_tokens(t.h, tok.data_ptr(), L.VDR_F32, Bt, S, tout.data_ptr(), vdr.OUT_CLS, L.VDR_F32,
                                          body.data_ptr(), body.numel(), stream)
        assert rc == VDR_ERR_WORKSPACE, (varlen, rc)
    torch.cuda.synchronize()
    assert len(ws.handed) == len(calls) and len(tws.handed) == 2
    for whole, _ in ws.handed + tws.handed:
        assert bool((whole == mg.CANARY).all()), "a refused call wrote to its workspace"
    for k, o in list(outs.items()) + [("tokens_cls", tout)]:
        assert bool((o.view(torch.uint8) == mg.CANARY).all()), f"a refused call wrote to its output {k}"
    # ... and the same calls with the whole workspace run
    ws.fill, ws.short = "ones", 0
    for name, call in calls.items():
        call()
        ws.check_guards(name)
    for k, o in outs.items():
        assert mg.canary_left(o) == 0 and torch.isfinite(o).all(), k


def workspace_fill_range(case, fill, lo, hi):
    """Localising a failure: run `case` with pattern `fill` over the fraction [lo, hi) of the body only and report whether
    the outputs still equal the untouched engine's.  Halve the range until one buffer of carve() remains."""
    ref = _reference(case)
    e, run = _maker(case)()
    ws = Workspaces(e)
    ws.fill, ws.lo, ws.hi = fill, lo, hi
    got = _snapshot(run())
    ws.check_guards(f"{case} [{lo}, {hi})")
    return all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(got, ref))
