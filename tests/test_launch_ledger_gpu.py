"""GPU: the launch ledger -- what every kind of forward enqueues, as the library's own profiler books it.

vdr_api.hip runs the transformer blocks of every model through one loop whose path-dependent steps (MX-fp8, folded
LayerNorm, explicit LayerNorm pre- / post-LN) are chosen once per call.  Nothing else in the suite pins the launch
SEQUENCE of a forward: outputs can stay inside their gates while a launch is added, dropped or booked under another class.
For each case below one forward runs with Engine.profile(True) and profile_read() is compared with
tests/ledger/forward_launch_ledger.json for every kernel class: `launches` equal, `flops` and `bytes` equal (the same
doubles summed in the same order: rel 1e-12 is the JSON round trip, nothing else).

The ledger is a RECORD of the library at the commit its header names, never of the code under test:
    python tests/test_launch_ledger_gpu.py --record tests/ledger/forward_launch_ledger.json --lib path/to/libvdr.so --commit <sha>
(--hashes FILE also writes a sha256 per output tensor, for a one-off bitwise A/B of two builds).  A change that means to
alter what a forward launches re-records it from the build that change is compared against and says so.

The cases are the smallest shapes that reach each branch of the block loop, the CLS tail, the CLS rows' bf16 MLP and
the SAM loop; the one large case (ViT-B width, two blocks, batch 100) is the smallest launch at which the 8-phase qkv /
fc1 engage (M = 19 700: 77 x 9 = 693 and 77 x 12 = 924 tiles of 256 x 256, at least 512 needed) and the statistics are
finalised by ln_finalize or by the producers instead of inside the consumer.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LEDGER = os.path.join(HERE, "ledger", "forward_launch_ledger.json")

if __name__ == "__main__":  # (--record: the paths tests/conftest.py sets up under pytest)
    for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "vit-deep-radiomics_amd"), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from oracle import sam_oracle as so  # noqa: E402
from oracle import vit_oracle as vo  # noqa: E402

pytestmark = pytest.mark.gpu

P16 = vo.VitCfg(64, 16, 3, 128, 2, 3, 512)                                       # test_model_gpu.SMALL["p16_d128"]
SWIGLU = vo.VitCfg(56, 14, 3, 128, 2, 2, 320 + 64, act="swiglu", layerscale=True)  # ... ["dinov2_swiglu_ls"]
VITB2 = vo.VitCfg(224, 16, 3, 768, 12, 2, 3072)                                  # ViT-B width, two blocks
POSTLN = vo.postln_cfg(64, 1, 2, 128)
SAM = so.SamCfg(img=160, patch=16, dim=64, heads=1, layers=3, mlp_hidden=128, window=4, global_idx=(1,), out_chans=64)
REG_GOLDENS = {"dinov3_hf_tiny": "dinov3", "dinov2reg_hf_tiny": "dinov2reg"}

P16_VARIANTS = {
    "fold": {}, "nofold": dict(ln_fold=False), "fp8": dict(fp8=1),
    "resid32_fold": dict(resid_fp32=True), "resid32_nofold": dict(resid_fp32=True, ln_fold=False),
    "ln_fin_fused": dict(ln_fin_fused=True), "full_last_block": dict(full_last_block=True),
    "mb2_streams2": dict(micro_batch=2, streams=2),  # batch 5: three micro-batches on two streams
}
SWIGLU_VARIANTS = {"fold": {}, "fp8": dict(fp8=1), "fp8_cls_bf16": dict(fp8=1, fp8_cls_bf16=True)}
PATHS = {"fold": {}, "nofold": dict(ln_fold=False), "fp8": dict(fp8=1)}


def _vit_engine(cfg, w, **kw):
    import vdr
    vc = vdr.VdrConfig(img=cfg.img, patch=cfg.patch, in_chans=cfg.in_chans, dim=cfg.dim, heads=cfg.heads, layers=cfg.layers,
                       mlp_hidden=cfg.mlp_hidden, act=cfg.act, pre_ln=cfg.pre_ln, layerscale=cfg.layerscale, has_cls=cfg.has_cls,
                       has_pos=cfg.has_pos, input_ln=cfg.input_ln, ln_eps=cfg.ln_eps, **kw)
    e = vdr.Engine(vc)
    e.load_weights(w)
    return e


def _images(cfg, kw, batch, mode):
    def make():
        e = _vit_engine(cfg, vo.make_weights(cfg, seed=3, scale=0.05), **kw)
        x = vo.make_images(cfg, batch, seed=4).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _layers(kw, last_all_cls):
    def make():
        import vdr
        e = _vit_engine(P16, vo.make_weights(P16, seed=3, scale=0.05), **kw)
        x = vo.make_images(P16, 5, seed=4).cuda()
        specs = [vdr.LayerOut(0, vdr.OUT_CLS), vdr.LayerOut(1, vdr.OUT_DENSE)]
        specs += [] if last_all_cls else [vdr.LayerOut(2, vdr.OUT_POOLED)]
        specs += [vdr.LayerOut(2, vdr.OUT_CLS)]
        return e, lambda: e.forward_layers(x, specs)
    return make


def _attn_maps(kw, with_tokens):
    def make():
        import vdr
        e = _vit_engine(P16, vo.make_weights(P16, seed=3, scale=0.05), **kw)
        x = vo.make_images(P16, 5, seed=4).cuda()
        maps = [vdr.AttnMap(0, q_rows=1), vdr.AttnMap(2, q_rows=e.n_tokens, head_mean=True)]
        outs = [vdr.LayerOut(1, vdr.OUT_TOKENS)] if with_tokens else []

        def run():
            feats, got = e.forward_attn_maps(x, maps, outs)
            return list(feats) + list(got)
        return e, run
    return make


def _postln(lens):
    def make():
        import vdr
        e = _vit_engine(POSTLN, vo.make_weights(POSTLN, seed=13, scale=0.05))
        x = vo.make_tokens(4, 17, POSTLN.dim, seed=14).cuda()
        return e, lambda: [e.forward_tokens(x, vdr.OUT_CLS, lengths=lens)]
    return make


def _registers(name, kw, mode):
    def make():
        import numpy as np
        import vdr
        import dinov3_ref as dr
        rc = dr.golden_cfg(np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False), REG_GOLDENS[name])
        e = vdr.Engine(dr.vdr_config(rc, **kw))
        e.load_weights(dr.make_weights(rc, seed=5))
        x = vo.make_images(rc.vit, 3, seed=6).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _sam(kw, mode):
    def make():
        import vdr
        c = SAM
        vc = vdr.VdrConfig(img=c.img, patch=c.patch, in_chans=3, dim=c.dim, heads=c.heads, layers=c.layers, mlp_hidden=c.mlp_hidden,
                           has_cls=False, has_pos=True, ln_eps=c.ln_eps, window=c.window, global_blocks=tuple(c.global_idx),
                           neck_chans=c.out_chans, **kw)
        e = vdr.Engine(vc)
        e.load_weights(so.make_weights(c, seed=21, scale=0.05))
        x = so.make_images(c, 2, seed=22).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _vitb2(kw):
    def make():
        import vdr
        e = _vit_engine(VITB2, vo.make_weights(VITB2, seed=71), **kw)
        x = torch.rand(100, 3, 224, 224, generator=torch.Generator().manual_seed(72)).to(torch.bfloat16).cuda()
        return e, lambda: [e.forward(x, vdr.OUT_TOKENS)]
    return make


def _cases():
    from vdr import _lib as L
    modes = {"cls": L.OUT_CLS, "tokens": L.OUT_TOKENS}
    cases = {}
    for v, kw in P16_VARIANTS.items():
        for mn, mode in modes.items():
            cases[f"p16_d128-{v}-{mn}"] = _images(P16, kw, 5, mode)
    for v, kw in SWIGLU_VARIANTS.items():
        for mn, mode in modes.items():
            cases[f"dinov2_swiglu_ls-{v}-{mn}"] = _images(SWIGLU, kw, 4, mode)
    for v, kw in PATHS.items():
        cases[f"layers-{v}-last_all_cls"] = _layers(kw, True)
        cases[f"layers-{v}-last_pooled_and_cls"] = _layers(kw, False)
        cases[f"attn_maps-{v}-maps_only"] = _attn_maps(kw, False)
        cases[f"attn_maps-{v}-maps_and_tokens"] = _attn_maps(kw, True)
    cases["postln-fixed"] = _postln(None)
    cases["postln-varlen"] = _postln([5, 1, 17, 9])
    for name in sorted(REG_GOLDENS):
        for v in ("fold", "nofold"):
            for mn, mode in modes.items():
                cases[f"{name}-{v}-{mn}"] = _registers(name, PATHS[v], mode)
    for v, kw in PATHS.items():
        cases[f"sam-{v}-neck"] = _sam(kw, L.OUT_ENCODER)
        cases[f"sam-{v}-tokens_only"] = _sam(kw, L.OUT_TOKENS)
    cases["vitb2_b100-fold"] = _vitb2({})
    cases["vitb2_b100-ln_fin_fused"] = _vitb2(dict(ln_fin_fused=True))
    return cases


CASE_IDS = (
    [f"p16_d128-{v}-{m}" for v in P16_VARIANTS for m in ("cls", "tokens")]
    + [f"dinov2_swiglu_ls-{v}-{m}" for v in SWIGLU_VARIANTS for m in ("cls", "tokens")]
    + [f"{k}-{v}-{t}" for v in PATHS for k, t in (("layers", "last_all_cls"), ("layers", "last_pooled_and_cls"),
                                                  ("attn_maps", "maps_only"), ("attn_maps", "maps_and_tokens"))]
    + ["postln-fixed", "postln-varlen"]
    + [f"{n}-{v}-{m}" for n in sorted(REG_GOLDENS) for v in ("fold", "nofold") for m in ("cls", "tokens")]
    + [f"sam-{v}-{t}" for v in PATHS for t in ("neck", "tokens_only")]
    + ["vitb2_b100-fold", "vitb2_b100-ln_fin_fused"]
)


def _run(make):
    """One profiled forward of a case: ({class: {launches, flops, bytes}}, the output tensors)."""
    e, forward = make()
    e.profile(True)
    outs = forward()
    torch.cuda.synchronize()
    prof = e.profile_read()
    e.profile(False)
    return {k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in prof.items()}, outs


@pytest.fixture(scope="module")
def ledger():
    with open(LEDGER) as f:
        return json.load(f)


def test_the_ledger_holds_exactly_the_cases(ledger):
    assert sorted(ledger["cases"]) == sorted(CASE_IDS) == sorted(_cases())
    assert len(ledger["recorded_at_commit"]) == 40


@pytest.mark.parametrize("case", CASE_IDS)
def test_forward_launches_match_the_ledger(ledger, case):
    got, _ = _run(_cases()[case])
    want = ledger["cases"][case]
    for k in sorted(set(got) | set(want)):
        print(f"{case} {k}: got {got.get(k)}  ledger {want.get(k)}")
    assert sorted(got) == sorted(want), "kernel classes with launches"
    for k in sorted(want):
        assert got[k]["launches"] == want[k]["launches"], (case, k)
        assert got[k]["flops"] == pytest.approx(want[k]["flops"], rel=1e-12, abs=0.0), (case, k)
        assert got[k]["bytes"] == pytest.approx(want[k]["bytes"], rel=1e-12, abs=0.0), (case, k)


def _record(argv):
    import argparse
    ap = argparse.ArgumentParser(description="record the launch ledger from a build of libvdr.so")
    ap.add_argument("--record", required=True, metavar="LEDGER.json")
    ap.add_argument("--lib", help="the libvdr.so to record from (default: the package's own)")
    ap.add_argument("--commit", required=True, help="the commit that library was built at (the ledger's header)")
    ap.add_argument("--hashes", metavar="FILE", help="also write `case index sha256` of every output tensor")
    a = ap.parse_args(argv)
    from vdr import _lib as L
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)  # before the first load(): every Engine of this process uses it
    cases, out, hashes = _cases(), {}, []
    assert sorted(cases) == sorted(CASE_IDS)
    for cid in CASE_IDS:
        out[cid], outs = _run(cases[cid])
        for i, t in enumerate(outs):
            h = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
            hashes.append(f"{cid} {i} {h}")
        print(cid, {k: v["launches"] for k, v in out[cid].items()}, flush=True)
    with open(a.record, "w") as f:
        json.dump({"recorded_at_commit": a.commit, "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.hashes:
        with open(a.hashes, "w") as f:
            f.write("\n".join(hashes) + "\n")


if __name__ == "__main__":
    _record(sys.argv[1:])
