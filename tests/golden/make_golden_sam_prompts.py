"""Goldens of SAM's point and mask prompts: transformers.SamModel (5.15.0) on the embeddings and decoder seeds of the box-prompt
goldens (sam_hf_decoder_{g8,g10}.npz; make_golden_sam_decoder.py), with the 11 prompt tensors the box path does not read drawn
by tests/sam_prompt_ref.py from a seed of their own.

    python tests/golden/make_golden_sam_prompts.py      -> tests/golden/sam_hf_prompts_{g8,g10}.npz, README_sam_prompts.md

Stored per prompt set: the prompts, pred_masks / iou_scores of all four mask tokens, and the measured differences of
tests/sam_prompt_ref.py's two modes from them (relative L2, worst absolute difference, worst IoU-head difference).  The gates of
the tests are derived from those as README_sam_decoder.md derives the box path's: GPU decode 2 x the bf16 mode's difference, CPU
4 x the float64 one.  Nothing comes from device output.  Condition, asserted here for every set: at most 10 % of a golden's own
logits lie within the absolute gate of zero (the mask-IoU check leaves out only those)."""
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
import sam_prompt_ref as PR  # noqa: E402

PSEED = {"g8": 21, "g10": 24}          # the prompt weights (tests/sam_prompt_ref.draw_prompt_weights)
# the seed each set's point positions (and random mask) are drawn with: the first of 0, 1, 2, .. at which the set meets the
# 10 % condition below -- found by running this file's measurement on the CPU, which is what the condition asks for
SETSEED = {("g8", "point1"): 1, ("g8", "points3"): 1, ("g10", "point1"): 3, ("g10", "points3"): 2, ("g10", "box_points2"): 1}


def hf_model(img, mlp_dim, w):
    """the decoder and prompt encoder of the box goldens' miniature SamModel; the vision tower is not run (image_embeddings are given)"""
    from transformers import SamConfig, SamMaskDecoderConfig, SamModel, SamPromptEncoderConfig, SamVisionConfig
    vc = SamVisionConfig(hidden_size=64, output_channels=256, num_hidden_layers=2, num_attention_heads=1, image_size=img,
                         patch_size=16, window_size=4, global_attn_indexes=[1], mlp_dim=128, layer_norm_eps=1e-6)
    m = SamModel(SamConfig(vision_config=vc, prompt_encoder_config=SamPromptEncoderConfig(image_size=img, patch_size=16),
                           mask_decoder_config=SamMaskDecoderConfig(mlp_dim=mlp_dim)))
    sd = m.state_dict()
    hf = R.to_hf(w)
    for k, v in hf.items():
        assert k in sd and sd[k].numel() == v.numel(), (k, tuple(v.shape))
        sd[k] = v.reshape(sd[k].shape)
    assert all(k in hf for k in sd if k.startswith(("prompt_encoder.", "mask_decoder."))), "a prompt / decoder tensor was not set"
    m.load_state_dict(sd)
    return m.eval()


def prompt_sets(tag, c):
    """name -> dict(boxes, points, labels, mask_input): the prompts in the library's shapes (mask_input [B, 4g, 4g]: per image)"""
    B, nb, img, g = c["emb"].shape[0], c["boxes"].shape[1], c["cfg"].img, c["cfg"].g

    def rs(name):
        return np.random.RandomState(1000 * PSEED[tag] + SETSEED.get((tag, name), 0))

    def pts(n, name):
        return torch.from_numpy(rs(name).uniform(4.0, img - 4.0, size=(B, nb, n, 2)).astype(np.float32))

    def lab(rows):
        return torch.tensor([rows[i % len(rows)] for i in range(B * nb)], dtype=torch.int32).reshape(B, nb, -1)
    sets = {
        "point1": dict(points=pts(1, "point1"), labels=lab([[1]])),                                       # T = 7, with the padding row
        "points3": dict(points=pts(3, "points3"), labels=lab([[1, 0, -1], [1, 1, 0]])),                    # T = 9
        "box_points2": dict(boxes=c["boxes"], points=pts(2, "box_points2"), labels=lab([[1, 0], [0, 1]])),     # T = 9
        # the refinement step: the box case's own single-mask logits (problem 0 of each image) as the image's mask prompt
        "box_refine": dict(boxes=c["boxes"], mask_input=c["pred_masks_single"][:, 0, 0].clone()),
    }
    if tag == "g10":
        sets["points10_mask"] = dict(points=pts(10, "points10_mask"), labels=lab([[1, 0, 1, 1, 0, -1, 1, 0, 0, 1], [0, 1, 1, 0, 1, 1, -1, -1, 0, 1]]),   # T = 16
                                     mask_input=c["pred_masks_single"][:, 0, 0].clone())   # (a noise mask fails the 10 % condition at every seed tried)
        sets["box_point_pad"] = dict(boxes=c["boxes"], points=pts(1, "box_point_pad"), labels=lab([[1], [-10], [0]]))
    return sets


def main():
    import transformers
    print("transformers", transformers.__version__)
    table = []
    for tag in ("g8", "g10"):
        c = R.golden_case(HERE, tag)
        w = dict(c["weights"])
        pw = PR.draw_prompt_weights(PSEED[tag])
        w.update(pw)
        cfg, emb = c["cfg"], c["emb"]
        m = hf_model(cfg.img, cfg.mlp_dim, w)
        out = dict(pseed=PSEED[tag], prompt_sha256=R.weights_sha256(pw), transformers=transformers.__version__)
        names = []
        for name, s in prompt_sets(tag, c).items():
            kw = {}
            if "boxes" in s:
                kw["input_boxes"] = s["boxes"].float()
            if "points" in s:
                kw["input_points"], kw["input_labels"] = s["points"].float(), s["labels"].long()
            if "mask_input" in s:
                kw["input_masks"] = s["mask_input"][:, None].float()
            with torch.no_grad():
                multi = m(image_embeddings=emb, multimask_output=True, **kw)
                single = m(image_embeddings=emb, multimask_output=False, **kw)
            all4 = torch.cat([single.pred_masks, multi.pred_masks], dim=2)
            iou4 = torch.cat([single.iou_scores, multi.iou_scores], dim=2)
            args = dict(boxes=s.get("boxes"), points=s.get("points"), labels=s.get("labels"), mask_input=s.get("mask_input"))
            f64 = R.diffs(*PR.decode(w, emb, cfg, mode="f64", **args), all4, iou4)
            b16 = R.diffs(*PR.decode(w, emb, cfg, mode="bf16", **args), all4, iou4)
            gate_abs = 2.0 * b16[1]
            near = float((all4.abs() < gate_abs).double().mean())
            T = 5 + (s["points"].shape[2] if "points" in s else 0) + (2 if "boxes" in s else 1)
            print(f"{tag} {name}: T {T} logits std {float(all4.std()):.3f}  f64 relL2 {f64[0]:.3e} max|d| {f64[1]:.3e} iou {f64[2]:.3e}  "
                  f"bf16 relL2 {b16[0]:.3e} max|d| {b16[1]:.3e} iou {b16[2]:.3e}  within the gate of 0: {near:.4f}")
            assert near <= 0.10, (tag, name, near)   # change the prompts or the seed, never the cap
            assert f64[0] < 1e-5, (tag, name, f64)   # the restatement IS transformers' arithmetic (fp32 against float64)
            names.append(name)
            for k, v in s.items():
                out[f"{name}.{k}"] = v.numpy()
            out[f"{name}.all4"], out[f"{name}.iou4"] = all4.numpy(), iou4.numpy()
            out[f"{name}.f64_diff"], out[f"{name}.bf16_diff"] = np.array(f64), np.array(b16)
            table.append((tag, name, T, f64, b16, near))
        out["names"] = ",".join(names)
        path = os.path.join(HERE, f"sam_hf_prompts_{tag}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    with open(os.path.join(HERE, "README_sam_prompts.md"), "w") as f:
        f.write("# Goldens of the point and mask prompts\n\n"
                "Written by `make_golden_sam_prompts.py` (transformers.SamModel on the embeddings and decoder seeds of\n"
                "`sam_hf_decoder_{g8,g10}.npz`; the 11 prompt tensors drawn by `tests/sam_prompt_ref.py`).  Each file stores the prompts,\n"
                "the outputs of all four mask tokens and the differences measured below; no weights, no embeddings.\n\n"
                "Gates, derived as `README_sam_decoder.md` derives the box path's: the restatement of `tests/sam_prompt_ref.py` is run\n"
                "on the CPU in its two modes against the golden.  The float64 mode differs by transformers' own fp32 rounding; the\n"
                "bf16 mode rounds wherever the device stores bf16, so its difference is what the device's number formats cost.  The\n"
                "GPU decode must stay within **2 x the bf16 mode's difference** (the device's fp32 sums associate differently), the\n"
                "CPU restatement within **4 x the float64 mode's** (another BLAS may sum in another order).  Nothing is derived from\n"
                "device output.  At most 10 % of a golden's logits may lie within the absolute gate of zero (asserted by the\n"
                "generator): the mask-IoU check leaves out only those pixels.\n\n"
                "Columns: relative L2 / worst absolute difference of the logits / worst difference of the IoU head.\n\n"
                "| case | prompt set | T | float64 mode | bf16 mode | GPU gate (2 x bf16) | logits within the gate of 0 |\n|---|---|---|---|---|---|---|\n")
        for tag, name, T, f64, b16, near in table:
            f.write(f"| {tag} | {name} | {T} | {f64[0]:.2e} / {f64[1]:.2e} / {f64[2]:.2e} | {b16[0]:.2e} / {b16[1]:.2e} / {b16[2]:.2e} | "
                    f"{2 * b16[0]:.2e} / {2 * b16[1]:.2e} / {2 * b16[2]:.2e} | {100 * near:.1f} % |\n")


if __name__ == "__main__":
    main()
