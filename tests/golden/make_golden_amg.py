"""Golden of the automatic mask generator's scoring: transformers (5.15.0) helpers on the miniature SamModel of the prompt goldens
(sam_hf_prompts_g8.npz: the embedding of image 0, the decoder seed and the prompt-weight seed of make_golden_sam_prompts.py).

    python tests/golden/make_golden_amg.py      -> tests/golden/sam_hf_amg_g8.npz, README_amg.md

A 4 x 4 point grid (transformers' _build_point_grid times the image side) is decoded by SamModel into three masks a point; the
masks are up-sampled to the image size with F.interpolate (bilinear, align_corners=False), and _compute_stability_score and
_batched_mask_to_box of transformers.models.sam.image_processing_pil_sam (the module that imports without torchvision) score
them.  _mask_to_rle encodes a few designed masks for MaskSet.rle.  Stored: the grid, SamModel's low-resolution logits and IoU
predictions, the three pixel counts, the stability scores, the boxes, the thresholds chosen below, the gates and the RLE cases.

Gates.  tests/sam_prompt_ref.py's decode is run on the CPU in its bf16 mode (it rounds wherever the device stores bf16) and
its logits are scored by vdr.amg.mask_stats_torch: the worst difference of a candidate's stability score, area and predicted
IoU from the golden's is what the device's number formats cost, and the GPU test allows 2 x that (README_amg.md).  The filter
decision is compared only for candidates whose predicted IoU and stability lie further from their thresholds than those gates;
the thresholds are chosen here -- from the reference alone -- so that at most a quarter of the candidates is left out and both
kept and dropped candidates exist among the rest.  Both are asserted.  Nothing comes from device output."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "vit-deep-radiomics_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import sam_prompt_ref as PR  # noqa: E402
from make_golden_sam_prompts import hf_model  # noqa: E402

N_PER_SIDE = 4


def rle_cases():
    """[5, 6, 5] bool: empty, full, first pixel set, a block, a checkerboard"""
    m = torch.zeros((5, 6, 5), dtype=torch.bool)
    m[1] = True
    m[2, 0, 0] = True
    m[3, 2:5, 1:3] = True
    m[4] = (torch.arange(6)[:, None] + torch.arange(5)[None, :]) % 2 == 0
    return m


def main():
    import transformers
    import transformers.models.sam.image_processing_pil_sam as hf
    from vdr import amg
    print("transformers", transformers.__version__)
    base, _ = PR.golden_prompts(HERE, "g8")
    cfg, w, emb = base["cfg"], base["weights"], base["emb"][:1]
    img = cfg.img
    grid = torch.from_numpy(hf._build_point_grid(N_PER_SIDE) * float(img)).to(torch.float32)
    assert torch.equal(grid, amg.point_grid(N_PER_SIDE, img))
    n = grid.shape[0]
    pts, lbl = grid.reshape(1, n, 1, 2), torch.ones((1, n, 1), dtype=torch.int64)
    m = hf_model(img, cfg.mlp_dim, w)
    with torch.no_grad():
        out = m(image_embeddings=emb, input_points=pts, input_labels=lbl, multimask_output=True)
    low, iou = out.pred_masks[0].float(), out.iou_scores[0].float()                     # [n, 3, 4g, 4g], [n, 3]
    offset = 1.0                                                                        # SAM's default; the miniature's logits have a spread of a few units
    up = torch.nn.functional.interpolate(low, size=(img, img), mode="bilinear", align_corners=False)
    stab = hf._compute_stability_score(up, 0.0, offset)
    n_hi = (up > 0.0 + offset).sum((-1, -2)).to(torch.int32)
    n_lo = (up > 0.0 - offset).sum((-1, -2)).to(torch.int32)
    n_mid = (up > 0.0).sum((-1, -2)).to(torch.int32)
    assert torch.equal(stab.isnan(), n_lo == 0) and torch.equal(stab[n_lo > 0], (n_hi / n_lo)[n_lo > 0])
    boxes = hf._batched_mask_to_box(up > 0.0).to(torch.int32)
    counts = torch.stack([n_hi, n_mid, n_lo], dim=-1)

    # the bf16 restatement on the CPU: what the device's number formats cost
    lg16, iou16 = PR.decode(w, emb, cfg, points=pts.float(), labels=lbl.to(torch.int32), mode="bf16")
    c16, b16 = amg.mask_stats_torch(lg16[0, :, 1:].reshape(-1, 4 * cfg.g, 4 * cfg.g).float(), (img, img), 0.0, offset)
    c16 = c16.reshape(n, 3, 3)
    s16 = amg.stability(c16)
    both = ~(stab.isnan() | s16.isnan())
    assert torch.equal(stab.isnan(), s16.isnan()), "a candidate empties at threshold - offset in one of the two: move the offset"
    d_stab = float((s16 - stab)[both].abs().max())
    d_area = int((c16[..., 1] - n_mid).abs().max())
    d_iou = float((iou16[0, :, 1:].float() - iou).abs().max())
    g_stab, g_area, g_iou = 2.0 * d_stab, 2 * d_area, 2.0 * d_iou
    print(f"logits std {float(low.std()):.3f} offset {offset}; bf16 restatement: stability {d_stab:.3e} area {d_area} px of {img * img} iou {d_iou:.3e}")

    # thresholds from the reference alone: the first pair of quantile mid-points that leaves out at most a quarter
    chosen = None
    flat_iou, flat_stab = iou.reshape(-1), stab.reshape(-1)
    si, ss = torch.sort(flat_iou).values, torch.sort(flat_stab[~flat_stab.isnan()]).values
    for qi in (0.5, 0.4, 0.6, 0.3, 0.7):
        for qs in (0.5, 0.4, 0.6, 0.3, 0.7):
            ki, ks = int(qi * (si.numel() - 1)), int(qs * (ss.numel() - 1))
            t_iou, t_stab = float((si[ki] + si[ki + 1]) / 2), float((ss[ks] + ss[ks + 1]) / 2)
            clear = ((flat_iou - t_iou).abs() > g_iou) & (flat_stab.isnan() | ((flat_stab - t_stab).abs() > g_stab))
            keep = (flat_iou > t_iou) & (flat_stab > t_stab)
            if float((~clear).double().mean()) <= 0.25 and int((keep & clear).sum()) >= 2 and int((~keep & clear).sum()) >= 2 and chosen is None:
                chosen = (t_iou, t_stab, clear, keep)
    assert chosen is not None, "no threshold pair leaves at most a quarter of the candidates out with kept and dropped ones among the rest"
    t_iou, t_stab, clear, keep = chosen
    assert float((~clear).double().mean()) <= 0.25 and int((keep & clear).sum()) >= 1 and int((~keep & clear).sum()) >= 1
    print(f"thresholds: iou {t_iou:.6f} stability {t_stab:.6f}: {int(keep.sum())} of {keep.numel()} kept, {int((~clear).sum())} left out of the comparison")

    rm = rle_cases()
    rle = hf._mask_to_rle(rm)
    rle_counts = np.concatenate([np.array(r["counts"], dtype=np.int64) for r in rle])
    rle_lens = np.array([len(r["counts"]) for r in rle], dtype=np.int64)
    assert all(r["size"] == [6, 5] for r in rle)

    path = os.path.join(HERE, "sam_hf_amg_g8.npz")
    np.savez_compressed(path, transformers=transformers.__version__, n_per_side=N_PER_SIDE, grid=grid.numpy(), low_res=low.numpy(), iou=iou.numpy(),
                        counts=counts.numpy(), stability=stab.numpy(), boxes=boxes.numpy(), offset=np.float64(offset),
                        pred_iou_thresh=np.float64(t_iou), stability_score_thresh=np.float64(t_stab),
                        gate_stability=np.float64(g_stab), gate_area=np.int64(g_area), gate_iou=np.float64(g_iou),
                        keep=keep.reshape(n, 3).numpy(), clear=clear.reshape(n, 3).numpy(),
                        rle_masks=rm.numpy(), rle_counts=rle_counts, rle_lens=rle_lens)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    with open(os.path.join(HERE, "README_amg.md"), "w") as f:
        f.write("# Golden of the automatic mask generator's scoring\n\n"
                "Written by `make_golden_amg.py`: transformers' `SamModel` (the miniature of `sam_hf_prompts_g8.npz`, image 0) decodes a\n"
                f"{N_PER_SIDE} x {N_PER_SIDE} point grid (`_build_point_grid` times the image side {img}) into three masks a point; the masks are up-sampled with\n"
                "`F.interpolate` (bilinear, `align_corners=False`) and scored by `_compute_stability_score` and `_batched_mask_to_box` of\n"
                "`transformers.models.sam.image_processing_pil_sam` (the module that imports without torchvision).  `_mask_to_rle` encodes\n"
                "five designed 6 x 5 masks for `MaskSet.rle`.  The file stores the grid, the low-resolution logits and IoU predictions, the\n"
                "counts, stability scores and boxes, the thresholds and gates below and the RLE cases; no weights, no embeddings.\n\n"
                f"The miniature's logits have a standard deviation of {float(low.std()):.3f}; the stability offset is SAM's default, {offset}.\n\n"
                "Gates: `tests/sam_prompt_ref.py`'s decode runs on the CPU in its bf16 mode (it rounds wherever the device stores bf16),\n"
                "`vdr.amg.mask_stats_torch` scores its logits, and the worst difference from the golden over the candidates is what the\n"
                "device's number formats cost.  The GPU test allows **2 x** that.  Nothing is derived from device output.\n\n"
                "| quantity | bf16 restatement's worst difference | GPU gate (2 x) |\n|---|---|---|\n"
                f"| stability score | {d_stab:.3e} | {g_stab:.3e} |\n| area (pixels of {img * img}) | {d_area} | {g_area} |\n| predicted IoU | {d_iou:.3e} | {g_iou:.3e} |\n\n"
                f"Thresholds, chosen from the reference alone: `pred_iou_thresh` = {t_iou:.6f}, `stability_score_thresh` = {t_stab:.6f}.  The filter\n"
                "decision is compared only for candidates whose predicted IoU and stability lie further from these than the gates:\n"
                f"{int((~clear).sum())} of {clear.numel()} candidates are left out (the generator asserts at most a quarter), {int((keep & clear).sum())} of the rest are kept and\n"
                f"{int((~keep & clear).sum())} dropped (it asserts that both exist).\n")


if __name__ == "__main__":
    main()
