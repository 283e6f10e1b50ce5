"""Generate dinov3_hf_tiny.npz / dinov3_hf_gated_hd64.npz / dinov2reg_hf_tiny.npz (run ONCE in the authoring container).

    python tests/golden/make_golden_dinov3.py

Architecture cross-check for the register-token models: the in-container ``transformers`` ``DINOv3ViTModel`` and
``Dinov2WithRegistersModel`` built from local Config objects (no download), filled with seeded weights through the FULL
model's ``state_dict`` (a free-standing ``DINOv3ViTRopePositionEmbedding`` has an uninitialised ``inv_freq``; the one
inside a constructed model is initialised), run on seeded [0, 1) images.  Each file holds the model's own ``state_dict``
under ``sd.<key>`` (the names ``vdr.weights.from_dinov3_vit_state_dict`` / ``from_dinov2_hf_state_dict`` translate), the
input ``x`` and transformers' outputs: data only.

  dinov3_hf_tiny.npz        D 64, 2 heads (head dim 32), 2 layers, FFN 128, img 32, patch 8, 4 registers, erf-GELU MLP:
                            last_hidden_state [B, 1 + 4 + 16, D] (after the final norm), pooler_output (its CLS row);
                            plus x_64x32 / last_hidden_state_64x32 / pooler_output_64x32 from a 64 x 32 (H x W) input
                            (no position table: the RoPE angles follow the grid)
  dinov3_hf_gated_hd64.npz  D 64, 1 head (head dim 64), gated MLP (gate_proj / up_proj / down_proj, SiLU), 1 register
  dinov2reg_hf_tiny.npz     Dinov2WithRegistersModel: D 64, 2 heads, 2 layers, FFN 128 (mlp_ratio 2), img 28, patch 14,
                            4 registers; native size only (upstream resamples pos_embed with antialias=True at other
                            sizes, which the library does not reproduce)
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
D, LAYERS, BATCH = 64, 2, 3


def seeded_state_dict(m, seed):
    """every tensor from its own numpy PCG64 stream keyed by (seed, index): LayerNorm weights 1 + 0.1 N, LayerNorm
    biases 0.1 N, LayerScale lambda1 1 + 0.1 N, everything else 0.05 N"""
    sd = {}
    for idx, (k, v) in enumerate(m.state_dict().items()):
        if not torch.is_floating_point(v):
            sd[k] = v
            continue
        z = np.random.Generator(np.random.PCG64([seed, idx])).standard_normal(size=tuple(v.shape), dtype=np.float32)
        norm = "norm" in k.split(".")[-2]
        if (norm and k.endswith(".weight")) or k.endswith("lambda1"):
            z = 1.0 + 0.1 * z
        elif norm:
            z = 0.1 * z
        else:
            z = 0.05 * z
        sd[k] = torch.from_numpy(np.ascontiguousarray(z.astype(np.float32)))
    return sd


def images(H, W, seed):
    return torch.rand((BATCH, 3, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def save(name, meta, sd, store):
    arrays = {"sd." + k: v.numpy() for k, v in sd.items() if torch.is_floating_point(v)}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **meta, **arrays, **store)
    print(name, meta, {k: v.shape for k, v in store.items()})


def gen_dinov3(name, heads, ffn, registers, gated, seed, img=32, patch=8, second=None):
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    cfg = DINOv3ViTConfig(hidden_size=D, intermediate_size=ffn, num_hidden_layers=LAYERS, num_attention_heads=heads,
                          image_size=img, patch_size=patch, num_register_tokens=registers, use_gated_mlp=gated,
                          hidden_act="silu" if gated else "gelu")
    m = DINOv3ViTModel(cfg).eval()
    sd = seeded_state_dict(m, seed)
    m.load_state_dict(sd)
    x = images(img, img, seed + 10)
    store = {"x": x.numpy()}
    with torch.no_grad():
        o = m(pixel_values=x)
        store.update(last_hidden_state=o.last_hidden_state.numpy(), pooler_output=o.pooler_output.numpy())
        if second:
            x2 = images(second[0], second[1], seed + 11)
            o2 = m(pixel_values=x2)
            tag = f"_{second[0]}x{second[1]}"
            store.update({"x" + tag: x2.numpy(), "last_hidden_state" + tag: o2.last_hidden_state.numpy(),
                          "pooler_output" + tag: o2.pooler_output.numpy()})
    meta = dict(dim=D, heads=heads, layers=LAYERS, ffn=ffn, img=img, patch=patch, registers=registers, gated=int(gated),
                batch=BATCH, ln_eps=float(cfg.layer_norm_eps), rope_theta=float(cfg.rope_theta))
    save(name, meta, sd, store)


def gen_dinov2reg():
    from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel
    heads, img, patch, registers = 2, 28, 14, 4
    cfg = Dinov2WithRegistersConfig(hidden_size=D, num_hidden_layers=LAYERS, num_attention_heads=heads, mlp_ratio=2,
                                    image_size=img, patch_size=patch, num_register_tokens=registers)
    m = Dinov2WithRegistersModel(cfg).eval()
    sd = seeded_state_dict(m, 93)
    m.load_state_dict(sd)
    x = images(img, img, 103)
    with torch.no_grad():
        o = m(pixel_values=x)
    meta = dict(dim=D, heads=heads, layers=LAYERS, ffn=2 * D, img=img, patch=patch, registers=registers, gated=0, batch=BATCH,
                ln_eps=float(cfg.layer_norm_eps))
    save("dinov2reg_hf_tiny", meta, sd,
         {"x": x.numpy(), "last_hidden_state": o.last_hidden_state.numpy(), "pooler_output": o.pooler_output.numpy()})


if __name__ == "__main__":
    gen_dinov3("dinov3_hf_tiny", heads=2, ffn=128, registers=4, gated=False, seed=91, second=(64, 32))
    gen_dinov3("dinov3_hf_gated_hd64", heads=1, ffn=128, registers=1, gated=True, seed=92)
    gen_dinov2reg()
