"""Helpers of the automatic-mask-generator tests (plain module, imported like knn_ref.py).  The torch statements of the two kernels
live in vdr/amg.py (mask_stats_torch, nms_torch); here are only

* `upsample_f64`: a brute-force float64 bilinear up-sampling (align_corners=False), loops over nothing but the definition;
* `near`: the number of reference pixels within a distance of a threshold (the count bound of the CPU tests);
* designed and random box sets for NMS, each with the kept list worked out by hand;
* `golden_amg`: tests/golden/sam_hf_amg_g8.npz (tests/golden/README_amg.md);
* `sam_model`: the miniature SAM handle of the prompt goldens."""
import contextlib
import os

import numpy as np
import torch


def upsample_f64(logits: torch.Tensor, size) -> torch.Tensor:
    """[P, H, W] -> [P, oh, ow] float64: src = (o + 0.5) * n_in / n_out - 0.5 clamped at 0, i0 = floor, the four-point blend"""
    x = logits.double()
    oh, ow = size

    def axis(n_in, n_out):
        src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
        i0 = src.floor().long().clamp_max(n_in - 1)
        return i0, (i0 + 1).clamp_max(n_in - 1), src - i0
    y0, y1, ly = axis(x.shape[1], oh)
    x0, x1, lx = axis(x.shape[2], ow)
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly)[None, :, None] + bot * ly[None, :, None]


def near(ref_up: torch.Tensor, threshold: float, dist: float) -> torch.Tensor:
    """[P]: the pixels of each reference plane within `dist` of `threshold`"""
    return ((ref_up.double() - threshold).abs() <= dist).sum((-1, -2))


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
def designed_boxes():
    """name -> (boxes [N, 4], scores [N], iou_threshold, the kept indices in NMS order)"""
    f = torch.tensor
    return {
        # four times the same box: the best-scored one stays (equal scores: the lowest index)
        "identical": (f([[1.0, 2.0, 9.0, 7.0]] * 4), f([0.5, 0.9, 0.9, 0.1]), 0.5, [1]),
        "disjoint": (f([[0.0, 0.0, 4.0, 4.0], [10.0, 0.0, 14.0, 4.0], [0.0, 10.0, 4.0, 14.0], [10.0, 10.0, 14.0, 14.0]]),
                     f([0.1, 0.4, 0.3, 0.2]), 0.0, [1, 2, 3, 0]),
        # A-B-C along x, 10 wide, shifted by 3: iou(A, B) = iou(B, C) = 7 / 13 > 0.5, iou(A, C) = 4 / 16.  A removes B; B, being
        # removed, removes nothing: C stays
        "chain": (f([[0.0, 0.0, 10.0, 10.0], [3.0, 0.0, 13.0, 10.0], [6.0, 0.0, 16.0, 10.0]]), f([0.9, 0.8, 0.7]), 0.5, [0, 2]),
        # equal scores everywhere: index order; 0 removes 1 (identical), 2 is far away
        "ties": (f([[0.0, 0.0, 8.0, 8.0], [0.0, 0.0, 8.0, 8.0], [20.0, 20.0, 28.0, 28.0]]), f([0.5, 0.5, 0.5]), 0.5, [0, 2]),
        # zero-area boxes: two identical points give 0 / 0 = NaN (no suppression); a point inside a box gives 0 / area = 0
        "zero_area": (f([[5.0, 5.0, 5.0, 5.0], [5.0, 5.0, 5.0, 5.0], [0.0, 0.0, 10.0, 10.0], [2.0, 3.0, 2.0, 9.0]]),
                      f([0.9, 0.8, 0.7, 0.6]), 0.0, [0, 1, 2, 3]),
        # [0, 8] x [0, 8] against [0, 8] x [0, 4]: inter 32, union 64, iou exactly 0.5: not above 0.5, kept; at 0.49 it goes
        "exact_half": (f([[0.0, 0.0, 8.0, 8.0], [0.0, 0.0, 8.0, 4.0]]), f([0.9, 0.8]), 0.5, [0, 1]),
        "below_half": (f([[0.0, 0.0, 8.0, 8.0], [0.0, 0.0, 8.0, 4.0]]), f([0.9, 0.8]), 0.49, [0]),
    }


def random_boxes(n: int, seed: int, extent: float = 64.0):
    """n boxes with heavy overlap (centres in a small extent, sides up to half of it) and scores with ties -> (boxes, scores)"""
    rs = np.random.RandomState(seed)
    c = rs.uniform(0.0, extent, size=(n, 2))
    s = rs.uniform(1.0, extent / 2, size=(n, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=1).astype(np.float32)
    point = rs.rand(n) < 0.03
    boxes[point, 2:] = boxes[point, :2]                                      # a few zero-area boxes
    dup = np.flatnonzero(rs.rand(n) < 0.05)
    boxes[dup] = boxes[rs.randint(0, n, size=dup.size)]                      # and a few exact copies
    scores = np.round(rs.uniform(0.0, 1.0, size=n), 2).astype(np.float32)   # two decimals: many equal scores
    return torch.from_numpy(boxes), torch.from_numpy(scores)


def disjoint_boxes(n: int):
    """n boxes of a grid that do not touch: nothing is suppressed (the serial worst case of the walk)"""
    i = torch.arange(n, dtype=torch.float32)
    x, y = (i % 64) * 4.0, (i // 64) * 4.0
    return torch.stack([x, y, x + 3.0, y + 3.0], dim=1), torch.linspace(1.0, 0.0, n)


# ---- the golden and its model -------------------------------------------------------------------------------------------------
def golden_amg(golden_dir):
    z = np.load(os.path.join(golden_dir, "sam_hf_amg_g8.npz"), allow_pickle=False)
    out = {k: torch.from_numpy(z[k]) for k in ("grid", "low_res", "iou", "counts", "stability", "boxes", "keep", "clear", "rle_masks")}
    out.update({k: float(z[k]) for k in ("offset", "pred_iou_thresh", "stability_score_thresh", "gate_stability", "gate_iou")})
    out["gate_area"], out["n_per_side"] = int(z["gate_area"]), int(z["n_per_side"])
    counts, lens = z["rle_counts"].tolist(), z["rle_lens"].tolist()
    out["rle"] = [counts[sum(lens[:i]):sum(lens[:i + 1])] for i in range(len(lens))]
    return out


@contextlib.contextmanager
def sam_model(base, name):
    """the miniature SAM handle whose decoder is the prompt golden's (tests/sam_prompt_ref.golden_prompts' base case)"""
    import handle_configs as hc
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(base["cfg"].img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS[name] = hc.sam_config(cfg)
    try:
        w = dict(so.make_weights(cfg, seed=base["wseed"], scale=0.05))
        w.update(base["weights"])
        yield vdr.load_model(name, weights=w, decoder_eps=base["eps"])
    finally:
        del vdr.ARCHS[name]
