"""Engine configs and engines of the oracle's model descriptions (TEST HELPER): the one builder of a vdr.VdrConfig from a
VitCfg / SamCfg, of a loaded vdr.Engine from either, and of a loaded model under a temporary vdr.ARCHS name, plus the
small configs that several files run (TINY, P16, SWIGLU, POSTLN, SAM).  Every GPU test file that builds an engine from an
oracle config goes through here; none keeps a builder of its own."""
import contextlib
import os

import numpy as np

from oracle import sam_oracle as so
from oracle import vit_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
REG_GOLDENS = {"dinov3_hf_tiny": "dinov3", "dinov2reg_hf_tiny": "dinov2reg"}

TINY = vo.VitCfg(32, 8, 3, 64, 1, 2, 128)                                        # the vit_hf_tiny network: 4 x 4 grid, N = 17
P16 = vo.VitCfg(64, 16, 3, 128, 2, 3, 512)                                       # test_model_gpu.SMALL["p16_d128"]
SWIGLU = vo.VitCfg(56, 14, 3, 128, 2, 2, 320 + 64, act="swiglu", layerscale=True)  # ... ["dinov2_swiglu_ls"]
POSTLN = vo.postln_cfg(64, 1, 2, 128)
SAM = so.SamCfg(img=160, patch=16, dim=64, heads=1, layers=3, mlp_hidden=128, window=4, global_idx=(1,), out_chans=64)


def vit_config(cfg, **kw):
    """the vdr.VdrConfig of an oracle VitCfg; kw adds the engine's own switches and may override a field (layers=...)"""
    import vdr
    return vdr.VdrConfig(**{**dict(img=cfg.img, patch=cfg.patch, in_chans=cfg.in_chans, dim=cfg.dim, heads=cfg.heads,
                                   layers=cfg.layers, mlp_hidden=cfg.mlp_hidden, act=cfg.act, pre_ln=cfg.pre_ln,
                                   layerscale=cfg.layerscale, has_cls=cfg.has_cls, has_pos=cfg.has_pos, input_ln=cfg.input_ln,
                                   ln_eps=cfg.ln_eps), **kw})


def sam_config(c, **kw):
    """the vdr.VdrConfig of an oracle SamCfg"""
    import vdr
    return vdr.VdrConfig(img=c.img, patch=c.patch, in_chans=3, dim=c.dim, heads=c.heads, layers=c.layers, mlp_hidden=c.mlp_hidden,
                         has_cls=False, has_pos=True, ln_eps=c.ln_eps, window=c.window, global_blocks=tuple(c.global_idx),
                         neck_chans=c.out_chans, **kw)


def _loaded(vc, weights):
    import vdr
    e = vdr.Engine(vc)
    e.load_weights(weights)
    return e


def engine(cfg, weights, **config_kw):
    """a vdr.Engine of an oracle VitCfg with `weights` loaded"""
    return _loaded(vit_config(cfg, **config_kw), weights)


def sam_engine(cfg, weights, **config_kw):
    """a vdr.Engine of an oracle SamCfg with `weights` loaded"""
    return _loaded(sam_config(cfg, **config_kw), weights)


def first_blocks(weights, layers):
    """the weights of a model cut to its first `layers` blocks (load_weights is strict)"""
    return {k: v for k, v in weights.items() if not k.startswith("blocks.") or int(k.split(".")[1]) < layers}


@contextlib.contextmanager
def registered_model(name, cfg=TINY, seed=21, scale=0.05, **load_kw):
    """vdr.load_model of cfg's seeded weights under the temporary vdr.ARCHS entry `name`"""
    import vdr
    vdr.ARCHS[name] = vit_config(cfg)
    try:
        yield vdr.load_model(name, weights=vo.make_weights(cfg, seed=seed, scale=scale), **load_kw)
    finally:
        del vdr.ARCHS[name]


def reg_cfg(name):
    """the dinov3_ref.RegCfg of one of REG_GOLDENS"""
    import dinov3_ref as dr
    return dr.golden_cfg(np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False), REG_GOLDENS[name])


def sized_sam(cfg, side):
    """the SamCfg of the same encoder built at another input side"""
    return so.SamCfg(side, cfg.patch, 3, cfg.dim, cfg.heads, cfg.layers, cfg.mlp_hidden, cfg.window, tuple(cfg.global_idx),
                     cfg.out_chans, cfg.ln_eps)
