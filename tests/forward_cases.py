"""The forwards whose launch sequence and memory contract are pinned (TEST HELPER): one maker per case -- () -> (engine,
run) -- shared by tests/test_launch_ledger_gpu.py (what each enqueues) and tests/test_workspace_contract_gpu.py (what each
writes).  The cases are the smallest shapes that reach each branch of the block loop; tests/test_launch_ledger_gpu.py's
docstring says why each is there."""
import torch

import handle_configs as hc
from handle_configs import P16, POSTLN, REG_GOLDENS, SAM, SWIGLU
from oracle import sam_oracle as so
from oracle import vit_oracle as vo

VITB2 = vo.VitCfg(224, 16, 3, 768, 12, 2, 3072)                                  # ViT-B width, two blocks

P16_VARIANTS = {
    "fold": {}, "nofold": dict(ln_fold=False), "fp8": dict(fp8=1),
    "resid32_fold": dict(resid_fp32=True), "resid32_nofold": dict(resid_fp32=True, ln_fold=False),
    "ln_fin_fused": dict(ln_fin_fused=True), "full_last_block": dict(full_last_block=True),
    "mb2_streams2": dict(micro_batch=2, streams=2),  # batch 5: three micro-batches on two streams
}
SWIGLU_VARIANTS = {"fold": {}, "fp8": dict(fp8=1), "fp8_cls_bf16": dict(fp8=1, fp8_cls_bf16=True)}
PATHS = {"fold": {}, "nofold": dict(ln_fold=False), "fp8": dict(fp8=1)}


def _images(cfg, kw, batch, mode):
    def make():
        e = hc.engine(cfg, vo.make_weights(cfg, seed=3, scale=0.05), **kw)
        x = vo.make_images(cfg, batch, seed=4).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _layers(kw, last_all_cls):
    def make():
        import vdr
        e = hc.engine(P16, vo.make_weights(P16, seed=3, scale=0.05), **kw)
        x = vo.make_images(P16, 5, seed=4).cuda()
        specs = [vdr.LayerOut(0, vdr.OUT_CLS), vdr.LayerOut(1, vdr.OUT_DENSE)]
        specs += [] if last_all_cls else [vdr.LayerOut(2, vdr.OUT_POOLED)]
        specs += [vdr.LayerOut(2, vdr.OUT_CLS)]
        return e, lambda: e.forward_layers(x, specs)
    return make


def _attn_maps(kw, with_tokens):
    def make():
        import vdr
        e = hc.engine(P16, vo.make_weights(P16, seed=3, scale=0.05), **kw)
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
        e = hc.engine(POSTLN, vo.make_weights(POSTLN, seed=13, scale=0.05))
        x = vo.make_tokens(4, 17, POSTLN.dim, seed=14).cuda()
        return e, lambda: [e.forward_tokens(x, vdr.OUT_CLS, lengths=lens)]
    return make


def _registers(name, kw, mode):
    def make():
        import vdr
        import dinov3_ref as dr
        rc = hc.reg_cfg(name)
        e = vdr.Engine(dr.vdr_config(rc, **kw))
        e.load_weights(dr.make_weights(rc, seed=5))
        x = vo.make_images(rc.vit, 3, seed=6).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _sam(kw, mode):
    def make():
        c = SAM
        e = hc.sam_engine(c, so.make_weights(c, seed=21, scale=0.05), **kw)
        x = so.make_images(c, 2, seed=22).cuda()
        return e, lambda: [e.forward(x, mode)]
    return make


def _vitb2(kw):
    def make():
        import vdr
        e = hc.engine(VITB2, vo.make_weights(VITB2, seed=71), **kw)
        x = torch.rand(100, 3, 224, 224, generator=torch.Generator().manual_seed(72)).to(torch.bfloat16).cuda()
        return e, lambda: [e.forward(x, vdr.OUT_TOKENS)]
    return make


def cases():
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
