"""Automatic mask generation with a SAM / MedSAM checkpoint (segment_anything's SamAutomaticMaskGenerator, one crop layer; filter
and box conventions pinned against transformers' generator helpers): a grid of one-point prompts, each decoded into three
masks; every candidate scored at image resolution by ONE fused kernel (vdr.ops.mask_stats: the stability score's two pixel
counts, the area and the box, from the low-resolution logits, the up-sampled plane never written); filtered; greedy box NMS on
the device (vdr.ops.nms); the kept points decoded again -- a problem's bits do not depend on the call it travels in, so the
candidate's logits come back bit for bit and memory stays at one batch.  model.generate_masks (vdr/model.py) is the entry point.

mask_stats_torch and nms_torch state the two kernels in plain torch on the CPU, operation by operation: the kernels are read
against them bit for bit.

Small-region removal (min_mask_region_area > 0, segment_anything's postprocess_small_regions) runs after the NMS on the device:
the kept masks are binarised at `size` (vdr.ops.mask_binarize, mask_stats' arithmetic), holes and then islands below the area
are removed at 8-connectivity (vdr.ops.mask_clean: connected components, csrc/components.hip), and a second box NMS prefers the
masks that needed no change.  Deviations there: "largest" ties go to the lowest root; parity with OpenCV's
connectedComponentsWithStats, which segment_anything calls, is unpinned (the rule is restated on scipy.ndimage.label).

Out of scope: crop layers (crop_n_layers > 0, and with them the near-crop-edge filter), several images per call, mask-level NMS,
fp8."""
from __future__ import annotations

import numpy as np
import torch

MAX_CANDIDATES = 4096  # vdr_op_nms takes at most this many boxes


# ---- the torch statements -------------------------------------------------------------------------------------------------------
def _axis(n_in: int, n_out: int):
    """(i0, i1, l0, l1) of every output index along one axis: include/vdr.h's rule, each operation one fp32 rounding"""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    src = (torch.arange(n_out, dtype=torch.float32) + 0.5) * scale - 0.5
    src = torch.where(src < 0, torch.zeros_like(src), src)
    i0 = src.to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    return i0, i1, l0, l1


def upsample_torch(logits: torch.Tensor, size) -> torch.Tensor:
    """[P, H, W] fp32 on the CPU -> [P, oh, ow]: v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d), every product and sum a
    separate fp32 operation (no fused multiply-add)"""
    x = logits.detach().to("cpu", torch.float32)
    oh, ow = (int(v) for v in size)
    y0, y1, ly0, ly1 = _axis(x.shape[1], oh)
    x0, x1, lx0, lx1 = _axis(x.shape[2], ow)
    top, bot = x[:, y0], x[:, y1]
    ta, tb = lx0 * top[:, :, x0], lx1 * top[:, :, x1]
    ba, bb = lx0 * bot[:, :, x0], lx1 * bot[:, :, x1]
    return ly0[None, :, None] * (ta + tb) + ly1[None, :, None] * (ba + bb)


def mask_stats_torch(logits: torch.Tensor, size, threshold: float = 0.0, offset: float = 1.0):
    """vdr_op_mask_stats in torch on the CPU: logits fp32 [P, H, W] -> (counts int32 [P, 3], box int32 [P, 4])"""
    oh, ow = (int(v) for v in size)
    thr = torch.tensor(float(threshold), dtype=torch.float32)
    off = torch.tensor(float(offset), dtype=torch.float32)
    t_hi, t_lo = thr + off, thr - off
    P = int(logits.shape[0])
    counts = torch.zeros((P, 3), dtype=torch.int32)
    box = torch.zeros((P, 4), dtype=torch.int32)
    for p in range(P):   # plane by plane: the up-sampled plane is the large thing here
        v = upsample_torch(logits[p:p + 1], (oh, ow))[0]
        m = v > thr
        counts[p] = torch.stack([(v > t_hi).sum(), m.sum(), (v > t_lo).sum()]).to(torch.int32)
        if bool(m.any()):
            ys, xs = m.any(dim=1).nonzero()[:, 0], m.any(dim=0).nonzero()[:, 0]
            box[p] = torch.stack([xs[0], ys[0], xs[-1], ys[-1]]).to(torch.int32)
    return counts, box


def stability(counts: torch.Tensor) -> torch.Tensor:
    """float(n_hi) / float(n_lo) of counts [.., 3] (transformers' _compute_stability_score: int32 / int32 in fp32; 0 / 0 is NaN)"""
    return counts[..., 0].to(torch.float32) / counts[..., 2].to(torch.float32)


def nms_torch(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float):
    """vdr_op_nms in torch on the CPU: boxes [N, 4] (x0, y0, x1, y1), scores [N] -> (kept int32 [N], -1 behind the kept indices;
    count int32 [1]).  torchvision's nms: area = (x1 - x0) * (y1 - y0), inter = max(min(x1) - max(x0), 0) * max(min(y1) - max(y0), 0),
    iou = inter / ((area_i + area_j) - inter), suppressed when iou > threshold (strict; a NaN does not suppress); the order is a
    stable descending sort of the scores."""
    b = boxes.detach().to("cpu", torch.float32)
    N = int(b.shape[0])
    order = torch.sort(scores.detach().cpu(), descending=True, stable=True).indices
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = torch.tensor(float(iou_threshold), dtype=torch.float32)
    removed = torch.zeros(N, dtype=torch.bool)
    kept = []
    for i in range(N):
        if removed[i]:
            continue
        kept.append(int(order[i]))
        w = (torch.minimum(b[i, 2], b[i + 1:, 2]) - torch.maximum(b[i, 0], b[i + 1:, 0])).clamp_min(0)
        h = (torch.minimum(b[i, 3], b[i + 1:, 3]) - torch.maximum(b[i, 1], b[i + 1:, 1])).clamp_min(0)
        inter = w * h
        iou = inter / ((area[i] + area[i + 1:]) - inter)
        removed[i + 1:] |= iou > thr
    out = torch.full((N,), -1, dtype=torch.int32)
    out[:len(kept)] = torch.tensor(kept, dtype=torch.int32)
    return out, torch.tensor([len(kept)], dtype=torch.int32)


def point_grid(n_per_side: int, size: int) -> torch.Tensor:
    """SAM's build_point_grid times the image side: [n * n, 2] (x, y) fp32, x fastest; computed in float64, rounded once"""
    if isinstance(n_per_side, bool) or int(n_per_side) != n_per_side or int(n_per_side) < 1:
        raise ValueError(f"point_grid: n_per_side must be a positive integer, got {n_per_side!r}")
    n = int(n_per_side)
    offset = 1 / (2 * n)
    one = np.linspace(offset, 1 - offset, n)
    pts = np.stack([np.tile(one[None, :], (n, 1)), np.tile(one[:, None], (1, n))], axis=-1).reshape(-1, 2)
    return torch.from_numpy(pts * float(size)).to(torch.float32)


# ---- the result -----------------------------------------------------------------------------------------------------------------
def mask_to_rle(masks: torch.Tensor) -> "list[dict]":
    """[K, h, w] bool -> pycocotools' uncompressed RLE, column-major, counts starting with the run of zeros (transformers'
    _mask_to_rle): host side"""
    m = masks.detach().cpu().numpy().astype(bool)
    out = []
    for k in range(m.shape[0]):
        h, w = m.shape[1:]
        flat = m[k].T.reshape(-1)
        change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
        edges = np.concatenate([[0], change, [h * w]])
        counts = np.diff(edges).tolist()
        if flat.size and flat[0]:
            counts = [0] + counts
        out.append({"size": [h, w], "counts": counts})
    return out


class MaskSet:
    """What generate_masks returns, K masks in NMS order (best predicted IoU first), all on the device:
    low_res_logits [K, 4g, 4g] fp32; iou, stability fp32 [K]; area int32 [K] (pixels above the threshold at `size`); boxes int32
    [K, 4] XYXY, inclusive, at `size`; points fp32 [K, 2] (x, y), the prompt of each mask in input pixels; point_index int64 [K]
    (into the grid), mask_index int64 [K] (0 .. 2: which of the point's three masks).  After small-region removal
    (min_mask_region_area > 0) the set also carries cleaned uint8 [K, h, w], the cleaned masks at `size`, and changed int32 [K]
    (bit 0: holes were filled, bit 1: islands were removed); area and boxes are then the cleaned masks', and masks(), label_map()
    and rle() give the cleaned planes -- at `size` only."""

    def __init__(self, low_res_logits, iou, stability, area, boxes, points, point_index, mask_index, input_size, size, mask_threshold,
                 cleaned=None, changed=None):
        self.low_res_logits, self.iou, self.stability, self.area, self.boxes = low_res_logits, iou, stability, area, boxes
        self.cleaned, self.changed = cleaned, changed
        self.points, self.point_index, self.mask_index = points, point_index, mask_index
        self.input_size, self.size, self.mask_threshold = tuple(int(v) for v in input_size), tuple(int(v) for v in size), float(mask_threshold)

    def __len__(self):
        return int(self.iou.shape[0])

    def masks(self, size=None) -> torch.Tensor:
        """[K, h, w] bool at the statistics' size or `size`: bilinear (align_corners=False) > mask_threshold; plain torch"""
        size = self.size if size is None else tuple(int(v) for v in size)
        if self.cleaned is not None:
            if size != self.size:
                raise ValueError(f"MaskSet.masks: the set was cleaned at {self.size} (min_mask_region_area); another size, {size}, would need cleaning again")
            return self.cleaned != 0
        if len(self) == 0:
            return torch.zeros((0, *size), dtype=torch.bool, device=self.low_res_logits.device)
        up = torch.nn.functional.interpolate(self.low_res_logits[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]
        return up > self.mask_threshold

    def boxes_xywh(self) -> torch.Tensor:
        """[K, 4] int32 (x, y, w, h) with w = x1 - x0, h = y1 - y0 (segment_anything's box_xyxy_to_xywh)"""
        b = self.boxes
        return torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], dim=1)

    def label_map(self, size=None) -> torch.Tensor:
        """[h, w] int32: 0 background, k + 1 where mask k (NMS rank) shows.  Painted from the largest area to the smallest, so a
        small region stays visible on a large one; equal areas in NMS rank order (the better one first, the later one on top)"""
        m = self.masks(size)
        out = torch.zeros(m.shape[1:], dtype=torch.int32, device=m.device)
        for k in torch.sort(self.area, descending=True, stable=True).indices.tolist():
            out[m[k]] = k + 1
        return out

    def rle(self, size=None) -> "list[dict]":
        return mask_to_rle(self.masks(size))


def check_generate(model, x, points_per_side, points_per_batch, thresholds: dict, min_mask_region_area=0):
    """Every refusal of generate_masks, before any device work -> x as [1, 3, S, S]"""
    from . import segment as sg
    if isinstance(min_mask_region_area, bool) or not isinstance(min_mask_region_area, int) or min_mask_region_area < 0:
        raise ValueError(f"generate_masks: min_mask_region_area must be an integer >= 0, got {min_mask_region_area!r}")
    sg._require(model, "generate_masks")
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise ValueError(f"generate_masks: one image [1, 3, S, S] or [3, S, S], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dim() == 3:
        x = x[None]
    if x.shape[0] != 1:
        raise ValueError(f"generate_masks: one image a call, got a batch of {x.shape[0]} (several images per call are out of scope)")
    if isinstance(points_per_side, bool) or not isinstance(points_per_side, int) or points_per_side < 1:
        raise ValueError(f"generate_masks: points_per_side must be a positive integer, got {points_per_side!r}")
    if isinstance(points_per_batch, bool) or not isinstance(points_per_batch, int) or not 1 <= points_per_batch <= 65535 // 3:
        raise ValueError(f"generate_masks: points_per_batch must be an integer in 1 .. {65535 // 3} (three planes a point, 65535 a statistics call; "
                         f"decode_masks itself takes 65535 problems), got {points_per_batch!r}")
    for name, v in thresholds.items():
        if not isinstance(v, (int, float)) or isinstance(v, bool) or v != v:
            raise ValueError(f"generate_masks: {name} must be a number, got {v!r}")
    if thresholds["stability_score_offset"] < 0:
        raise ValueError(f"generate_masks: stability_score_offset must be >= 0, got {thresholds['stability_score_offset']!r}")
    if not model.mask_decoder.has_point_prompts:
        raise ValueError("generate_masks: the checkpoint has no point-prompt weights (point_embeddings.0/1, not_a_point_embed): weights absent")
    return x


def generate(model, x, points_per_side, points_per_batch, pred_iou_thresh, stability_score_thresh, stability_score_offset, mask_threshold,
             box_nms_thresh, size, min_mask_region_area=0) -> MaskSet:
    from . import ops
    x = check_generate(model, x, points_per_side, points_per_batch, dict(
        pred_iou_thresh=pred_iou_thresh, stability_score_thresh=stability_score_thresh, stability_score_offset=stability_score_offset,
        mask_threshold=mask_threshold, box_nms_thresh=box_nms_thresh), min_mask_region_area)
    img, dev = model.cfg.img, model.device
    size = (img, img) if size is None else ops.check_out_size("generate_masks", size)
    grid = point_grid(points_per_side, img).to(dev)
    n = int(grid.shape[0])
    emb = model.image_encoder(x)

    def decode(points):   # [k, 2] -> the three masks of every point: vdr.Segmentation [1, k, 3, 4g, 4g]
        k = int(points.shape[0])   # (clone: a slice of the grid need not start on the 16-byte boundary the decode asks of its pointers)
        return model.decode_masks(emb, points=points.reshape(1, k, 1, 2).clone(), point_labels=torch.ones((1, k, 1), dtype=torch.int32, device=dev),
                                  multimask=True)

    ious, counts, boxes = [], [], []
    for s0 in range(0, n, points_per_batch):   # no host synchronisation in this loop; a batch's logits are dropped
        seg = decode(grid[s0:s0 + points_per_batch])
        c, b, _ = seg.stats(size, mask_threshold, stability_score_offset)
        ious.append(seg.iou[0]), counts.append(c[0]), boxes.append(b[0])
    iou, counts, boxes = torch.cat(ious).reshape(-1), torch.cat(counts).reshape(-1, 3), torch.cat(boxes).reshape(-1, 4)   # candidate = 3 point + mask
    stab = stability(counts)
    flags = (iou > pred_iou_thresh) & (stab > stability_score_thresh)   # both strict; a NaN stability fails
    cand = flags.cpu().nonzero()[:, 0].to(dev)                           # host read 1: the flags
    g4 = 4 * model.mask_decoder.g

    def result(sel, logits):
        return MaskSet(logits, iou[sel], stab[sel], counts[sel, 1], boxes[sel], grid[sel // 3], sel // 3, sel % 3, (img, img), size, mask_threshold)
    if cand.numel() == 0:
        ms = result(cand, torch.zeros((0, g4, g4), dtype=torch.float32, device=dev))
        if min_mask_region_area > 0:
            ms.cleaned, ms.changed = torch.zeros((0, *size), dtype=torch.uint8, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)
        return ms
    if cand.numel() > MAX_CANDIDATES:
        raise ValueError(f"generate_masks: {cand.numel()} candidates pass the filters, NMS takes at most {MAX_CANDIDATES}: raise pred_iou_thresh "
                         "or stability_score_thresh, or lower points_per_side")
    kept, count = ops.nms(boxes[cand].to(torch.float32), iou[cand], box_nms_thresh)
    sel = cand[kept[:int(count.cpu())].long()]                           # host read 2: the count
    logits = []
    for s0 in range(0, int(sel.numel()), points_per_batch):             # the kept points again: the same bits, whatever the batch
        part = sel[s0:s0 + points_per_batch]
        lg = decode(grid[part // 3]).low_res_logits[0]                   # [k, 3, 4g, 4g]
        logits.append(torch.gather(lg, 1, (part % 3)[:, None, None, None].expand(-1, 1, g4, g4))[:, 0])
    ms = result(sel, torch.cat(logits))
    return remove_small_regions(ms, min_mask_region_area, box_nms_thresh) if min_mask_region_area > 0 else ms


def remove_small_regions(ms: MaskSet, min_area: int, box_nms_thresh: float) -> MaskSet:
    """segment_anything's postprocess_small_regions on a MaskSet of K >= 1 masks: the masks binarised at ms.size; holes, then islands,
    below min_area removed at 8-connectivity; boxes from the cleaned masks; a second box NMS whose score is 1 for a mask that
    needed no change and 0 for one that did (visited in a stable order: unchanged masks first, each class in rank order), so
    that a changed mask goes when it now overlaps an unchanged one.  The survivors stay in their rank order (best predicted IoU
    first); a changed mask takes its new area and box.  One more host read: the second NMS count."""
    from . import ops, segment as sg
    cleaned, changed, stats = sg.clean_planes("generate_masks", ms.low_res_logits, ms.size, ms.mask_threshold, min_area, holes=True, islands=True,
                                              largest=False, connectivity=8)
    score = (changed == 0).to(torch.float32)
    kept, count = ops.nms(stats[:, 1:].to(torch.float32), score, box_nms_thresh)
    keep = torch.sort(kept[:int(count.cpu())].long()).values
    return MaskSet(ms.low_res_logits[keep], ms.iou[keep], ms.stability[keep], stats[keep, 0], stats[keep, 1:], ms.points[keep], ms.point_index[keep],
                   ms.mask_index[keep], ms.input_size, ms.size, ms.mask_threshold, cleaned=cleaned[keep].view(torch.uint8), changed=changed[keep])
