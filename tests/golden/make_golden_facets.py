"""Generate tests/golden/vit_hf_facets.npz (run ONCE in the authoring container; provenance: README_facets.md).

    python tests/golden/make_golden_facets.py

The recipe of vit_hf_tiny (make_golden.py: transformers ViTModel built from a local ViTConfig, eps 1e-6, the oracle's
seeded weights, no download), batch 2, with forward hooks on every layer's attention query / key / value Linear -- what
dino-vit-features' ViTExtractor hooks for its facets -- and output_hidden_states for the `token` facet (the raw residual
stream after each layer, before the final LayerNorm).  Both layers of the tiny model are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import vit_oracle as vo  # noqa: E402

QKV_NAMES = {"query": ("attention.query", "attention.q_proj"), "key": ("attention.key", "attention.k_proj"),
             "value": ("attention.value", "attention.v_proj")}


def main(img=32, patch=8, dim=64, heads=1, layers=2, ffn=128, batch=2, wseed=21, xseed=6):
    from transformers import ViTConfig, ViTModel

    cfg = vo.VitCfg(img, patch, 3, dim, heads, layers, ffn, ln_eps=1e-6)
    w = vo.make_weights(cfg, seed=wseed, scale=0.05)
    hc = ViTConfig(hidden_size=dim, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn, image_size=img,
                   patch_size=patch, layer_norm_eps=1e-6, hidden_act="gelu", hidden_dropout_prob=0.0,
                   attention_probs_dropout_prob=0.0)
    m = ViTModel(hc, add_pooling_layer=False)
    sd = m.state_dict()
    sd["embeddings.cls_token"] = w["cls_token"]
    sd["embeddings.position_embeddings"] = w["pos_embed"]
    sd["embeddings.patch_embeddings.projection.weight"] = w["patch_embed.proj.weight"]
    sd["embeddings.patch_embeddings.projection.bias"] = w["patch_embed.proj.bias"]
    names = dict(m.named_modules())
    hooked = {}
    for i in range(layers):
        s = f"blocks.{i}."
        lin = {}
        for f, suffixes in QKV_NAMES.items():
            # (the Linear's name differs between transformers versions: ...{i}.attention.attention.query / ...{i}.attention.q_proj)
            hit = [n for n in names if any(n.endswith(f".{i}.{sfx}") or n.endswith(f".{i}.attention.{sfx}") for sfx in suffixes)]
            assert len(hit) == 1, (i, f, hit)
            lin[f] = hit[0]
        hooked[i] = lin
        d = lin["query"].rsplit(".", 1)[0].rsplit(".attention", 1)[0] + "."  # the layer's prefix
        q, k, v = w[s + "attn.qkv.weight"].chunk(3, dim=0)
        qb, kb, vb = w[s + "attn.qkv.bias"].chunk(3, dim=0)
        for f, ww, bb in (("query", q, qb), ("key", k, kb), ("value", v, vb)):
            sd[lin[f] + ".weight"], sd[lin[f] + ".bias"] = ww.clone(), bb.clone()
        proj = [n for n in sd if n.startswith(d) and n.endswith(".weight") and ("o_proj" in n or "output.dense" in n) and "attention" in n]
        assert len(proj) == 1, proj
        sd[proj[0]], sd[proj[0][:-6] + "bias"] = w[s + "attn.proj.weight"], w[s + "attn.proj.bias"]
        for a, b in (("layernorm_before", "norm1"), ("layernorm_after", "norm2")):
            sd[d + a + ".weight"], sd[d + a + ".bias"] = w[s + b + ".weight"], w[s + b + ".bias"]
        fc = {k_: k_ for k_ in sd if k_.startswith(d) and "attention" not in k_ and "layernorm" not in k_}
        fc1 = sorted(k_ for k_ in fc if k_.endswith(".weight") and sd[k_].shape == (ffn, dim))
        fc2 = sorted(k_ for k_ in fc if k_.endswith(".weight") and sd[k_].shape == (dim, ffn))
        assert len(fc1) == 1 and len(fc2) == 1, (fc1, fc2)
        sd[fc1[0]], sd[fc1[0][:-6] + "bias"] = w[s + "mlp.fc1.weight"], w[s + "mlp.fc1.bias"]
        sd[fc2[0]], sd[fc2[0][:-6] + "bias"] = w[s + "mlp.fc2.weight"], w[s + "mlp.fc2.bias"]
    sd["layernorm.weight"], sd["layernorm.bias"] = w["norm.weight"], w["norm.bias"]
    for k_, v_ in sd.items():
        assert m.state_dict()[k_].shape == v_.shape, (k_, m.state_dict()[k_].shape, v_.shape)
    m.load_state_dict(sd)
    m.eval()
    got = {}
    handles = []
    for i, lin in hooked.items():
        for f, n in lin.items():
            handles.append(names[n].register_forward_hook(lambda mod, inp, out, key=f"{f}.{i}": got.__setitem__(key, out.detach().clone())))
    x = vo.make_images(cfg, batch, seed=xseed)
    with torch.no_grad():
        o = m(pixel_values=x, output_hidden_states=True)
    for h in handles:
        h.remove()
    hs = o.hidden_states
    assert len(hs) == layers + 1
    for i in range(layers):
        got[f"token.{i}"] = hs[i + 1]
    arrays = {k_: v_.reshape(batch, -1, dim).numpy().astype(np.float32) for k_, v_ in got.items()}
    # the stored tokens of vit_hf_tiny are this model's last_hidden_state: the two goldens describe the same network
    tiny = np.load(os.path.join(HERE, "vit_hf_tiny.npz"))
    assert np.array_equal(tiny["tokens"], o.last_hidden_state.numpy())
    np.savez_compressed(os.path.join(HERE, "vit_hf_facets.npz"), img=img, patch=patch, dim=dim, heads=heads, layers=layers, ffn=ffn,
                        batch=batch, wseed=wseed, xseed=xseed, wscale=0.05, **arrays)
    import descriptor_ref as dref
    ref = dref.facets(dref.plain(cfg), w, x)
    for k_, v_ in sorted(arrays.items()):
        f, i = k_.split(".")
        err = float((ref[f][int(i)] - torch.from_numpy(v_)).abs().max())
        print(f"vit_hf_facets {k_}: {v_.shape} max|restatement - hf| = {err:.3e}")
        assert err < 2.5e-6, (k_, err)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
