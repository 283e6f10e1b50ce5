"""Generate clip_hf_tiny.npz / siglip_hf_tiny.npz (run ONCE in the authoring container).

    python tests/golden/make_golden_clip.py

Architecture cross-check for the vision towers of language-supervised models: the in-container ``transformers``
``CLIPVisionModelWithProjection`` and ``SiglipVisionModel`` built from local Config objects (no download), filled with
seeded weights, run on seeded [0, 1) images.  Each file holds the model's own ``state_dict`` under ``sd.<key>`` (the
names ``vdr.weights.from_clip_vision_state_dict`` / ``from_siglip_vision_state_dict`` translate), the input ``x`` and
transformers' outputs: data only.

  clip_hf_tiny.npz    D 64, 2 heads, 2 layers, FFN 128, img 32, patch 8, projection 48, hidden_act quick_gelu:
                      last_hidden_state (the encoder output, BEFORE post_layernorm), pooler_output
                      (post_layernorm of the CLS row), image_embeds; plus x_64x32 and last_hidden_state_64x32 /
                      image_embeds_64x32 from a 64 x 32 (H x W) input with interpolate_pos_encoding=True
  siglip_hf_tiny.npz  same sizes, hidden_act gelu_pytorch_tanh: last_hidden_state (AFTER post_layernorm),
                      pooler_output (the attention-pooling head); plus the 64 x 32 pair
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
D, HEADS, LAYERS, FFN, IMG, PATCH, PROJ, BATCH = 64, 2, 2, 128, 32, 8, 48, 3


def seeded_state_dict(m, seed):
    """every tensor from its own numpy PCG64 stream keyed by (seed, index): LayerNorm weights 1 + 0.1 N, LayerNorm
    biases 0.1 N, embeddings (class / position / probe) 0.02 N, everything else 0.05 N"""
    sd = {}
    for idx, (k, v) in enumerate(m.state_dict().items()):
        if not torch.is_floating_point(v):
            sd[k] = v  # (position_ids buffers)
            continue
        z = np.random.Generator(np.random.PCG64([seed, idx])).standard_normal(size=tuple(v.shape), dtype=np.float32)
        norm = "norm" in k.split(".")[-2]
        if norm and k.endswith(".weight"):
            z = 1.0 + 0.1 * z
        elif norm:
            z = 0.1 * z
        elif "embedding" in k.split(".")[-1] or "position_embedding" in k or k.endswith("probe"):
            z = 0.02 * z
        else:
            z = 0.05 * z
        sd[k] = torch.from_numpy(np.ascontiguousarray(z.astype(np.float32)))
    return sd


def images(H, W, seed):
    return torch.rand((BATCH, 3, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def save(name, m, sd, store):
    arrays = {"sd." + k: v.numpy() for k, v in sd.items() if torch.is_floating_point(v)}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), dim=D, heads=HEADS, layers=LAYERS, ffn=FFN, img=IMG, patch=PATCH,
                        proj=PROJ, batch=BATCH, ln_eps=float(m.config.layer_norm_eps), **arrays, **store)
    print(name, "ln_eps", m.config.layer_norm_eps, "hidden_act", m.config.hidden_act, {k: v.shape for k, v in store.items()})


def gen_clip():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=D, intermediate_size=FFN, projection_dim=PROJ, num_hidden_layers=LAYERS,
                           num_attention_heads=HEADS, image_size=IMG, patch_size=PATCH, hidden_act="quick_gelu",
                           attention_dropout=0.0)
    m = CLIPVisionModelWithProjection(cfg).eval()
    sd = seeded_state_dict(m, 71)
    m.load_state_dict(sd)
    x, x2 = images(IMG, IMG, 81), images(64, 32, 82)
    with torch.no_grad():
        o = m(pixel_values=x)
        o2 = m(pixel_values=x2, interpolate_pos_encoding=True)
        pooled = m.vision_model(pixel_values=x).pooler_output
    save("clip_hf_tiny", m, sd, {
        "x": x.numpy(), "last_hidden_state": o.last_hidden_state.numpy(), "pooler_output": pooled.numpy(),
        "image_embeds": o.image_embeds.numpy(), "x_64x32": x2.numpy(),
        "last_hidden_state_64x32": o2.last_hidden_state.numpy(), "image_embeds_64x32": o2.image_embeds.numpy()})


def gen_siglip():
    from transformers import SiglipVisionConfig, SiglipVisionModel
    cfg = SiglipVisionConfig(hidden_size=D, intermediate_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                             image_size=IMG, patch_size=PATCH, hidden_act="gelu_pytorch_tanh", attention_dropout=0.0)
    m = SiglipVisionModel(cfg).eval()
    sd = seeded_state_dict(m, 72)
    m.load_state_dict(sd)
    x, x2 = images(IMG, IMG, 91), images(64, 32, 92)
    with torch.no_grad():
        o = m(pixel_values=x)
        o2 = m(pixel_values=x2, interpolate_pos_encoding=True)
    save("siglip_hf_tiny", m, sd, {
        "x": x.numpy(), "last_hidden_state": o.last_hidden_state.numpy(), "pooler_output": o.pooler_output.numpy(),
        "x_64x32": x2.numpy(), "last_hidden_state_64x32": o2.last_hidden_state.numpy(),
        "pooler_output_64x32": o2.pooler_output.numpy()})


if __name__ == "__main__":
    gen_clip()
    gen_siglip()
