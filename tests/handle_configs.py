"""Engine configs of the oracle's model descriptions, shared by the handle tests (TEST HELPER): tests/test_weight_slots_gpu.py,
tests/test_handle_lifetime_gpu.py."""
import os

import numpy as np

from oracle import sam_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
REG_GOLDENS = {"dinov3_hf_tiny": "dinov3", "dinov2reg_hf_tiny": "dinov2reg"}  # (as tests/test_launch_ledger_gpu.py)


def vit_config(cfg, **kw):
    """the vdr.VdrConfig of an oracle VitCfg"""
    import vdr
    return vdr.VdrConfig(img=cfg.img, patch=cfg.patch, in_chans=cfg.in_chans, dim=cfg.dim, heads=cfg.heads, layers=cfg.layers,
                         mlp_hidden=cfg.mlp_hidden, act=cfg.act, pre_ln=cfg.pre_ln, layerscale=cfg.layerscale, has_cls=cfg.has_cls,
                         has_pos=cfg.has_pos, input_ln=cfg.input_ln, ln_eps=cfg.ln_eps, **kw)


def sam_config(c, **kw):
    """the vdr.VdrConfig of an oracle SamCfg"""
    import vdr
    return vdr.VdrConfig(img=c.img, patch=c.patch, in_chans=3, dim=c.dim, heads=c.heads, layers=c.layers, mlp_hidden=c.mlp_hidden,
                         has_cls=False, has_pos=True, ln_eps=c.ln_eps, window=c.window, global_blocks=tuple(c.global_idx),
                         neck_chans=c.out_chans, **kw)


def reg_cfg(name):
    """the dinov3_ref.RegCfg of one of REG_GOLDENS"""
    import dinov3_ref as dr
    return dr.golden_cfg(np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False), REG_GOLDENS[name])


def sized_sam(cfg, side):
    """the SamCfg of the same encoder built at another input side"""
    return so.SamCfg(side, cfg.patch, 3, cfg.dim, cfg.heads, cfg.layers, cfg.mlp_hidden, cfg.window, tuple(cfg.global_idx),
                     cfg.out_chans, cfg.ln_eps)
