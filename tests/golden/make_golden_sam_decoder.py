"""Goldens of SAM's box-prompt encoder + mask decoder: transformers.SamModel (5.15.0) with a miniature vision tower and the
REAL decoder geometry (256 channels, 8 heads, depth 2, 4 mask tokens, upscale 64 / 32, IoU head depth 3; mlp_dim cut to 128).

    python tests/golden/make_golden_sam_decoder.py      -> tests/golden/sam_hf_decoder_{g8,g10}.npz

The decoder weights are NOT stored (2 M parameters): tests/sam_decoder_ref.py draws them from numpy.random.RandomState(seed);
each file stores the seed and the SHA-256 of the drawn bytes.  The vision tower's weights are oracle/sam_oracle.py's seeded
ones.  Stored per case: the configuration, the images, the neck embedding, the boxes, pred_masks / iou_scores for
multimask_output True and False, and the measured differences of tests/sam_decoder_ref.py's two modes from them (the
gates of the tests are derived from those; README_sam_decoder.md).

transformers applies its config's layer_norm_eps (1e-6) to the decoder's LayerNorms, segment_anything nn.LayerNorm's 1e-5;
the goldens are transformers', so the restatement and the library are given sam_decoder_ref.HF_EPS here."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "vit-deep-radiomics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sam_decoder_ref as R  # noqa: E402
from oracle import sam_oracle as so  # noqa: E402

MLP_DIM = 128
CASES = {
    # tag: (img, B, boxes [B, nb, 4] in pixels, decoder seed, encoder weight seed, image seed)
    "g8": (128, 2, [[[20.0, 30.0, 90.0, 100.0]], [[5.0, 8.0, 120.0, 60.0]]], 11, 3, 5),
    # n = 100 cells: no multiple of any tile; the second box is degenerate (x0 == x1)
    "g10": (160, 1, [[[30.0, 40.0, 120.0, 130.0], [80.0, 20.0, 80.0, 140.0], [0.0, 0.0, 159.0, 159.0]]], 12, 4, 6),
}


def encoder_cfg(img):
    return so.SamCfg(img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)


def hf_model(img, dec_w, enc_w):
    from transformers import SamConfig, SamMaskDecoderConfig, SamModel, SamPromptEncoderConfig, SamVisionConfig
    vc = SamVisionConfig(hidden_size=64, output_channels=256, num_hidden_layers=2, num_attention_heads=1, image_size=img,
                         patch_size=16, window_size=4, global_attn_indexes=[1], mlp_dim=128, layer_norm_eps=1e-6)
    m = SamModel(SamConfig(vision_config=vc, prompt_encoder_config=SamPromptEncoderConfig(image_size=img, patch_size=16),
                           mask_decoder_config=SamMaskDecoderConfig(mlp_dim=MLP_DIM)))
    sd = m.state_dict()
    pre = "vision_encoder."
    sd[pre + "pos_embed"] = enc_w["pos_embed"]
    sd[pre + "patch_embed.projection.weight"] = enc_w["patch_embed.proj.weight"]
    sd[pre + "patch_embed.projection.bias"] = enc_w["patch_embed.proj.bias"]
    for i in range(2):
        s_, d = f"blocks.{i}.", pre + f"layers.{i}."
        for j in (1, 2):
            sd[d + f"layer_norm{j}.weight"], sd[d + f"layer_norm{j}.bias"] = enc_w[s_ + f"norm{j}.weight"], enc_w[s_ + f"norm{j}.bias"]
        for k in ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "rel_pos_h", "rel_pos_w"):
            sd[d + "attn." + k] = enc_w[s_ + "attn." + k]
        for a, b in (("lin1", "fc1"), ("lin2", "fc2")):
            sd[d + f"mlp.{a}.weight"], sd[d + f"mlp.{a}.bias"] = enc_w[s_ + f"mlp.{b}.weight"], enc_w[s_ + f"mlp.{b}.bias"]
    sd[pre + "neck.conv1.weight"] = enc_w["neck.0.weight"]
    sd[pre + "neck.layer_norm1.weight"], sd[pre + "neck.layer_norm1.bias"] = enc_w["neck.1.weight"], enc_w["neck.1.bias"]
    sd[pre + "neck.conv2.weight"] = enc_w["neck.2.weight"]
    sd[pre + "neck.layer_norm2.weight"], sd[pre + "neck.layer_norm2.bias"] = enc_w["neck.3.weight"], enc_w["neck.3.bias"]
    hf = R.to_hf(dec_w)
    for k, v in hf.items():
        assert k in sd and sd[k].shape == v.shape, (k, tuple(v.shape))
        sd[k] = v
    m.load_state_dict(sd)
    return m.eval()


def diffs(lg, iou, ref_lg, ref_iou):
    d = (lg - ref_lg).double()
    return float(d.norm() / ref_lg.double().norm()), float(d.abs().max()), float((iou - ref_iou).abs().max())


def main():
    import transformers
    print("transformers", transformers.__version__)
    for tag, (img, B, boxes, dseed, wseed, xseed) in CASES.items():
        g = img // 16
        cfg = encoder_cfg(img)
        enc_w = so.make_weights(cfg, seed=wseed, scale=0.05)
        dec_w = R.draw_weights(dseed, MLP_DIM)
        m = hf_model(img, dec_w, enc_w)
        x = so.make_images(cfg, B, seed=xseed)
        bx = torch.tensor(boxes, dtype=torch.float32)
        with torch.no_grad():
            emb = m.get_image_embeddings(x)
            multi = m(image_embeddings=emb, input_boxes=bx, multimask_output=True)
            single = m(image_embeddings=emb, input_boxes=bx, multimask_output=False)
        all4 = torch.cat([single.pred_masks, multi.pred_masks], dim=2).double()      # [B, nb, 4, 4g, 4g]
        iou4 = torch.cat([single.iou_scores, multi.iou_scores], dim=2).double()
        rc = R.Cfg(g, img, MLP_DIM, **R.HF_EPS)
        f64 = diffs(*R.decode(dec_w, emb, bx, rc, "f64"), all4, iou4)
        b16 = diffs(*R.decode(dec_w, emb, bx, rc, "bf16"), all4, iou4)
        # the whole path.  |device - golden| <= |decoder(e) - exact decoder(e)| + |exact decoder(e) - exact decoder(golden emb)|
        # for the device's embedding e: the first term is the decoder's own gate, the second the effect of the encoder's bf16
        # error on the outputs, measured here with the float64 restatement on the embedding of the encoder's bf16-emulating
        # restatement (`enc_effect`).  `whole`: both modes at once, for the record (the two errors partly cancel in it)
        emb_em = so.sam_forward(cfg, enc_w, x, emulate_bf16=True)["out"]
        enc_effect = diffs(*R.decode(dec_w, emb_em, bx, rc, "f64"), *R.decode(dec_w, emb, bx, rc, "f64"))
        whole = diffs(*R.decode(dec_w, emb_em, bx, rc, "bf16"), all4, iou4)
        gate_abs = 2.0 * b16[1]
        near = float((all4.abs() < gate_abs).double().mean())
        print(f"sam_hf_decoder_{tag}: logits std {float(all4.std()):.3f} range [{float(all4.min()):.2f}, {float(all4.max()):.2f}]"
              f"  f64 restatement relL2 {f64[0]:.3e} max|d| {f64[1]:.3e} iou {f64[2]:.3e}"
              f"  bf16 mode relL2 {b16[0]:.3e} max|d| {b16[1]:.3e} iou {b16[2]:.3e}  encoder effect relL2 {enc_effect[0]:.3e} max|d| {enc_effect[1]:.3e} iou {enc_effect[2]:.3e}  both relL2 {whole[0]:.3e} max|d| {whole[1]:.3e} iou {whole[2]:.3e}  within the gate of 0: {near:.4f}")
        assert near < 0.10, (tag, near)  # the reference's own logits have spread: the mask IoU test leaves out < 10 % of pixels
        np.savez_compressed(os.path.join(HERE, f"sam_hf_decoder_{tag}.npz"), img=img, g=g, batch=B, mlp_dim=MLP_DIM,
                            ln_eps=R.HF_EPS["ln_eps"], final_ln_eps=R.HF_EPS["final_ln_eps"], ln2d_eps=R.HF_EPS["ln2d_eps"],
                            dseed=dseed, wseed=wseed, xseed=xseed, sha256=R.weights_sha256(dec_w),
                            transformers=transformers.__version__, image=x.numpy(), emb=emb.numpy(), boxes=bx.numpy(),
                            pred_masks_multi=multi.pred_masks.numpy(), iou_multi=multi.iou_scores.numpy(),
                            pred_masks_single=single.pred_masks.numpy(), iou_single=single.iou_scores.numpy(),
                            f64_diff=np.array(f64), bf16_diff=np.array(b16), whole_diff=np.array(whole), enc_effect=np.array(enc_effect))


if __name__ == "__main__":
    main()
