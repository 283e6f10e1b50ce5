"""Generate sam_hf_resize.npz + README_sam_resize.md (run ONCE in the authoring container).

    python tests/golden/make_golden_sam_resize.py

The architecture cross-check of make_golden.py's gen_sam_hf (the in-container ``transformers`` ``SamVisionModel`` built
from a local Config object, no download, loaded with the oracle's seeded weights), built at input sizes OTHER than the one
the position tables were learned at.  ``SamVisionModel(image_size=s)`` owns ``rel_pos_h / rel_pos_w`` of length
2 (s / patch) - 1 in its global blocks; here those parameters are REPLACED by the native-length tables, so transformers'
own ``get_rel_pos`` resamples them in every forward (F.interpolate, mode="linear").  transformers does not resample the
absolute ``pos_embed``; it gets the table ``vdr.weights.interpolate_pos_embed`` makes (bicubic, float64, one rounding),
the rule segment_anything-based code applies when it loads a 1024^2 checkpoint into a smaller encoder.

Each case holds seeds, the native and the new geometry and the first KEEP channels of transformers' output
``last_hidden_state[:, :KEEP]`` ([B, KEEP, g, g]; the neck ends in a LayerNorm2d, every channel is of the same kind):
data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))

from oracle import sam_oracle as so  # noqa: E402
from vdr.weights import interpolate_rel_pos, sam_tables_at  # noqa: E402

KEEP = 24
WSCALE = 0.05

# (native side, new side, window, dim, heads, layers, ffn, global blocks, out_chans, batch, wseed, xseed)
CASES = [
    (224, 64, 7, 128, 2, 2, 256, (1,), 64, 1, 51, 61),    # grid 14 -> 4: inside one zero-padded window
    (224, 112, 7, 128, 2, 2, 256, (1,), 64, 1, 52, 62),   # -> 7: one exact window
    (224, 144, 7, 128, 2, 2, 256, (1,), 64, 1, 53, 63),   # -> 9: padded windows, a grid side no kernel was instantiated for
    (224, 192, 7, 128, 2, 2, 256, (1,), 64, 1, 54, 64),   # -> 12
    (224, 320, 7, 128, 2, 3, 256, (0, 2), 64, 1, 55, 65), # -> 20: upsampled tables, two global blocks
    (160, 96, 4, 64, 1, 3, 128, (1,), 64, 1, 56, 66),     # grid 10 -> 6, window 4
    (160, 240, 4, 64, 1, 3, 128, (1,), 64, 1, 57, 67),    # -> 15
]


def cfgs(case):
    native, side, window, dim, heads, layers, ffn, gidx, oc, batch, wseed, xseed = case
    mk = lambda img: so.SamCfg(img, 16, 3, dim, heads, layers, ffn, window, tuple(gidx), oc, 1e-6)  # noqa: E731
    return mk(native), mk(side)


def hf_model(cfg, w_sized, w_native):
    """SamVisionModel at cfg.img with w_sized (pos_embed at the new grid), global rel-pos parameters = native tables."""
    from transformers import SamVisionConfig, SamVisionModel
    hc = SamVisionConfig(hidden_size=cfg.dim, output_channels=cfg.out_chans, num_hidden_layers=cfg.layers,
                         num_attention_heads=cfg.heads, image_size=cfg.img, patch_size=cfg.patch, window_size=cfg.window,
                         global_attn_indexes=list(cfg.global_idx), mlp_dim=cfg.mlp_hidden, layer_norm_eps=1e-6,
                         use_abs_pos=True, use_rel_pos=True, qkv_bias=True, hidden_act="gelu", attention_dropout=0.0)
    m = SamVisionModel(hc)
    sd = m.state_dict()
    pre = "vision_encoder."
    w = w_sized
    sd[pre + "pos_embed"] = w["pos_embed"]
    sd[pre + "patch_embed.projection.weight"] = w["patch_embed.proj.weight"]
    sd[pre + "patch_embed.projection.bias"] = w["patch_embed.proj.bias"]
    for i in range(cfg.layers):
        s_, d = f"blocks.{i}.", pre + f"layers.{i}."
        sd[d + "layer_norm1.weight"], sd[d + "layer_norm1.bias"] = w[s_ + "norm1.weight"], w[s_ + "norm1.bias"]
        sd[d + "layer_norm2.weight"], sd[d + "layer_norm2.bias"] = w[s_ + "norm2.weight"], w[s_ + "norm2.bias"]
        for k in ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "rel_pos_h", "rel_pos_w"):
            sd[d + "attn." + k] = w[s_ + "attn." + k]
        sd[d + "mlp.lin1.weight"], sd[d + "mlp.lin1.bias"] = w[s_ + "mlp.fc1.weight"], w[s_ + "mlp.fc1.bias"]
        sd[d + "mlp.lin2.weight"], sd[d + "mlp.lin2.bias"] = w[s_ + "mlp.fc2.weight"], w[s_ + "mlp.fc2.bias"]
    sd[pre + "neck.conv1.weight"] = w["neck.0.weight"]
    sd[pre + "neck.layer_norm1.weight"], sd[pre + "neck.layer_norm1.bias"] = w["neck.1.weight"], w["neck.1.bias"]
    sd[pre + "neck.conv2.weight"] = w["neck.2.weight"]
    sd[pre + "neck.layer_norm2.weight"], sd[pre + "neck.layer_norm2.bias"] = w["neck.3.weight"], w["neck.3.bias"]
    m.load_state_dict(sd)
    # the native-length tables in place of the sized ones: transformers' get_rel_pos resamples them itself
    for i in cfg.global_idx:
        attn = m.vision_encoder.layers[i].attn
        attn.rel_pos_h = torch.nn.Parameter(w_native[f"blocks.{i}.attn.rel_pos_h"].clone())
        attn.rel_pos_w = torch.nn.Parameter(w_native[f"blocks.{i}.attn.rel_pos_w"].clone())
    return m.eval()


def main():
    import transformers
    store, worst = {"n_cases": len(CASES), "keep": KEEP, "wscale": WSCALE}, 0.0
    for n, case in enumerate(CASES):
        native, side, window, dim, heads, layers, ffn, gidx, oc, batch, wseed, xseed = case
        cn, cs = cfgs(case)
        w0 = so.make_weights(cn, seed=wseed, scale=WSCALE)
        ws = sam_tables_at(w0, cs.grid, cs.global_idx)
        x = so.make_images(cs, batch, seed=xseed)
        with torch.no_grad():
            out = hf_model(cs, ws, w0)(pixel_values=x).last_hidden_state
        err = (so.sam_forward(cs, ws, x)["out"] - out).abs().max().item()
        worst = max(worst, err)
        print(f"case {n}: {native} -> {side} (grid {cn.grid} -> {cs.grid}, window {window}, global {gidx}): out {tuple(out.shape)} "
              f"max|oracle - hf| = {err:.3e}")
        assert err < 1e-4, err
        p = f"c{n}_"
        store.update({p + "native": native, p + "side": side, p + "window": window, p + "dim": dim, p + "heads": heads,
                      p + "layers": layers, p + "ffn": ffn, p + "global_idx": np.array(gidx), p + "out_chans": oc,
                      p + "batch": batch, p + "wseed": wseed, p + "xseed": xseed,
                      p + "out": out[:, :KEEP].contiguous().numpy()})
    # the identity case of the rule (no file entry needed: L == L0 returns the table)
    t = torch.randn(27, 64)
    assert torch.equal(interpolate_rel_pos(t, 27), t)
    path = os.path.join(HERE, "sam_hf_resize.npz")
    np.savez_compressed(path, **store)
    with open(os.path.join(HERE, "README_sam_resize.md"), "w") as f:
        f.write("# sam_hf_resize.npz\n\n"
                "Written by `make_golden_sam_resize.py` (see its docstring): `transformers.SamVisionModel` built at input sizes\n"
                "other than the one the oracle's seeded tables have, its global `rel_pos_h / rel_pos_w` parameters replaced by\n"
                "the native-length tables (transformers' `get_rel_pos` resamples them), `pos_embed` resampled by\n"
                "`vdr.weights.interpolate_pos_embed`.  Seeds, geometry and the first `keep` output channels per case; data only.\n\n"
                f"- torch {torch.__version__}, transformers {transformers.__version__}, numpy {np.__version__}\n"
                f"- cases (native side -> new side, window, global blocks): "
                + "; ".join(f"{c[0]} -> {c[1]}, {c[2]}, {c[7]}" for c in CASES) + "\n"
                f"- max |oracle/sam_oracle.sam_forward (host-resampled tables) - transformers| over the cases: {worst:.1e} "
                "(gate 1e-4)\n"
                f"- file size: {os.path.getsize(path)} bytes\n")
    print("wrote", path, os.path.getsize(path), "bytes; worst", worst)


if __name__ == "__main__":
    main()
