"""Generate dinov2_hf_resize.npz / vit_hf_resize.npz (run ONCE in the authoring container).

    python tests/golden/make_golden_resize.py

The architecture cross-check of make_golden.py (gen_dinov2_hf / gen_vit_hf: the in-container ``transformers``
``Dinov2Model`` / ``ViTModel`` built from local Config objects, no download, loaded with the oracle's seeded weights),
run at input sizes OTHER than the one the position table was learned at: transformers resamples
``position_embeddings`` inside the model (``interpolate_pos_encoding``: bicubic, align_corners=False, size=(gh, gw)).
``Dinov2Model`` always does; ``ViTModel`` is called with ``interpolate_pos_encoding=True``.

Each file holds seeds, the native geometry, the list of (H, W) and transformers' ``last_hidden_state`` per size
(``tokens_{H}x{W}``): data only.  Sizes: the native one, a larger and a smaller square, both rectangular orientations.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))

from oracle import vit_oracle as vo  # noqa: E402
from vdr.weights import interpolate_pos_embed  # noqa: E402

BATCH = 2


def images(chans, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((BATCH, chans, H, W), generator=g, dtype=torch.float32)


def hf_state_dict(m, w, layers, dinov2):
    """the oracle's canonical names -> the transformers module's (as make_golden.py's gen_vit_hf / gen_dinov2_hf)"""
    sd = m.state_dict()
    sd["embeddings.cls_token"] = w["cls_token"]
    sd["embeddings.position_embeddings"] = w["pos_embed"]
    sd["embeddings.patch_embeddings.projection.weight"] = w["patch_embed.proj.weight"]
    sd["embeddings.patch_embeddings.projection.bias"] = w["patch_embed.proj.bias"]
    for i in range(layers):
        s = f"blocks.{i}."
        d = f"encoder.layer.{i}." if dinov2 else f"layers.{i}."
        q, k, v = w[s + "attn.qkv.weight"].chunk(3, dim=0)
        qb, kb, vb = w[s + "attn.qkv.bias"].chunk(3, dim=0)
        names = ("query", "key", "value") if dinov2 else ("q_proj", "k_proj", "v_proj")
        pre = d + ("attention.attention." if dinov2 else "attention.")
        for nm, ww, bb in zip(names, (q, k, v), (qb, kb, vb)):
            sd[pre + nm + ".weight"] = ww.clone()
            sd[pre + nm + ".bias"] = bb.clone()
        out = d + ("attention.output.dense." if dinov2 else "attention.o_proj.")
        sd[out + "weight"] = w[s + "attn.proj.weight"]
        sd[out + "bias"] = w[s + "attn.proj.bias"]
        n1, n2 = ("norm1", "norm2") if dinov2 else ("layernorm_before", "layernorm_after")
        for src, dst in (("norm1", n1), ("norm2", n2)):
            sd[d + dst + ".weight"] = w[s + src + ".weight"]
            sd[d + dst + ".bias"] = w[s + src + ".bias"]
        if dinov2:
            sd[d + "layer_scale1.lambda1"] = w[s + "ls1.gamma"]
            sd[d + "layer_scale2.lambda1"] = w[s + "ls2.gamma"]
            sd[d + "mlp.weights_in.weight"] = w[s + "mlp.w12.weight"]
            sd[d + "mlp.weights_in.bias"] = w[s + "mlp.w12.bias"]
            sd[d + "mlp.weights_out.weight"] = w[s + "mlp.w3.weight"]
            sd[d + "mlp.weights_out.bias"] = w[s + "mlp.w3.bias"]
        else:
            for n in ("fc1", "fc2"):
                sd[d + f"mlp.{n}.weight"] = w[s + f"mlp.{n}.weight"]
                sd[d + f"mlp.{n}.bias"] = w[s + f"mlp.{n}.bias"]
    sd["layernorm.weight"] = w["norm.weight"]
    sd["layernorm.bias"] = w["norm.bias"]
    return sd


def gen(name, dinov2, img, patch, dim, heads, layers, sizes, wseed, xseed, mlp_ratio=4):
    from transformers import Dinov2Config, Dinov2Model, ViTConfig, ViTModel

    if dinov2:
        ffn = (int(dim * mlp_ratio * 2 / 3) + 7) // 8 * 8  # transformers' Dinov2SwiGLUFFN hidden width
        cfg = vo.VitCfg(img, patch, 3, dim, heads, layers, ffn, act="swiglu", layerscale=True, ln_eps=1e-6)
        m = Dinov2Model(Dinov2Config(hidden_size=dim, num_hidden_layers=layers, num_attention_heads=heads, mlp_ratio=mlp_ratio,
                                     image_size=img, patch_size=patch, use_swiglu_ffn=True, layer_norm_eps=1e-6,
                                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0))
    else:
        ffn = mlp_ratio * dim
        cfg = vo.VitCfg(img, patch, 3, dim, heads, layers, ffn, ln_eps=1e-6)
        m = ViTModel(ViTConfig(hidden_size=dim, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn,
                               image_size=img, patch_size=patch, layer_norm_eps=1e-6, hidden_act="gelu",
                               hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False)
    w = vo.make_weights(cfg, seed=wseed, scale=0.05)
    m.load_state_dict(hf_state_dict(m, w, layers, dinov2))
    m.eval()
    store = {}
    for k, (H, W) in enumerate(sizes):
        x = images(3, H, W, xseed + k)
        with torch.no_grad():
            hs = (m(pixel_values=x) if dinov2 else m(pixel_values=x, interpolate_pos_encoding=True)).last_hidden_state
        store[f"tokens_{H}x{W}"] = hs.numpy()
        # sanity: the unchanged oracle, fed the float64-resampled table, agrees right now
        ws = dict(w)
        ws["pos_embed"] = interpolate_pos_embed(w["pos_embed"], (H // patch, W // patch))
        err = (vo.forward_images(cfg, ws, x)["tokens"] - hs).abs().max().item()
        print(f"{name} {H}x{W}: tokens {tuple(hs.shape)} max|oracle-hf| = {err:.3e}")
        assert err < 5e-5, err
    np.savez_compressed(os.path.join(HERE, name + ".npz"), img=img, patch=patch, dim=dim, heads=heads, layers=layers,
                        ffn=ffn, batch=BATCH, wseed=wseed, xseed=xseed, wscale=0.05,
                        sizes=np.asarray(sizes, dtype=np.int64), **store)


if __name__ == "__main__":
    # image k of a file: torch.rand([BATCH, 3, H, W]) from torch.Generator().manual_seed(xseed + k)
    # (mlp_ratio 3: a SwiGLU hidden width of 128, a multiple of 64 as the device GEMMs want it)
    gen("dinov2_hf_resize", True, 56, 14, 64, 1, 2, [(56, 56), (112, 112), (28, 28), (84, 112), (112, 70)], 31, 41, mlp_ratio=3)
    gen("vit_hf_resize", False, 64, 16, 64, 1, 2, [(64, 64), (128, 128), (32, 32), (96, 160), (160, 96)], 32, 51)
