"""Prompt in, mask out: SAM's prompt encoder (boxes, points, a dense mask prompt) and mask decoder on the neck output of the
library's SAM / MedSAM encoder (segment_anything's PromptEncoder + MaskDecoder; parity pinned against transformers.SamModel).

A "problem" is one (image, box) pair; P = B * nb, n = g * g cells.  The decode is ONE call of the library's decoder object
(vdr_mask_decode, include/vdr.h): a fixed chain of launches on the caller's stream -- the same number for every B and nb
(MaskDecoder.LAUNCHES) -- of the mask decoder kernels (cross_attention, token_linear, mask_upscale), the GEMM for the
image-side linears and LayerNorm, in a workspace the caller owns.  Per block the three projections that read the image side
(k and v of token-to-image, q of image-to-token) are ONE GEMM on the stacked weight [384, 256]; the positional-encoding terms
pe W^T + b of k and q are fp32 tables of n rows, computed once per decoder in float64 and added inside the attention kernel's
loads.

Points and the mask prompt go through vdr_mask_decode_prompts (the same 52 launches): tokens [iou; 4 mask tokens; np points;
one padding point if there is no box; 2 box corners if there is one], at most 16 per problem; with a mask prompt the keys
are bf16(emb + mask_downscaling(mask)) from ONE fused kernel (vdr_op_mask_embed).  propagate_masks (vdr/model.py) carries a
mask through a volume from one annotated slice: each slice's box is vdr_op_mask_box of its neighbour's logits.

The automatic mask generator (a grid of point prompts, fused mask statistics, box NMS) is vdr/amg.py.

Out of scope: per-problem point counts other than by label -1 padding, fp8.  MedSAM fine-tuned
the decoder with box prompts only: its point / mask-prompt weights are SAM's, nothing is claimed about their masks."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

SA_EPS = dict(ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6)   # segment_anything: nn.LayerNorm's default; LayerNorm2d 1e-6
HF_EPS = dict(ln_eps=1e-6, final_ln_eps=1e-5, ln2d_eps=1e-6)   # transformers.SamModel applies its config's layer_norm_eps


def clean_planes(what: str, logits, size, threshold=0.0, min_area=0, holes=True, islands=True, largest=False, connectivity=8, max_planes=64,
                 lead=None):
    """Binarise planes of low-resolution logits at `size` and clean them: logits fp32 [P, h, w] or [G, M, h, w] on the device
    (read in place) -> (masks bool [.., oh, ow], changed int32 [..], stats int32 [.., 5]).  ONE vdr.ops.mask_binarize and ONE
    vdr.ops.mask_clean per chunk of at most max_planes planes, so that the label workspace stays bounded (8 bytes a pixel);
    every refusal comes before any device work.  lead: the leading shape of the results when it is
    not the logits' own (a [B, nb, M, h, w] decode passed as [B nb, M, h, w])."""
    from . import components as cc, ops
    oh, ow = ops.check_out_size(what, size)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError(f"{what}: threshold must be a number, got {threshold!r}")
    min_area, mode, connectivity = cc.check_clean(what, min_area, holes, islands, largest, connectivity)
    if isinstance(max_planes, bool) or not isinstance(max_planes, int) or not 1 <= max_planes <= 65535:
        raise ValueError(f"{what}: max_planes must be an integer in 1 .. 65535, got {max_planes!r}")
    lead = tuple(int(v) for v in (logits.shape[:-2] if lead is None else lead))
    groups = logits if logits.dim() == 4 else logits[:, None]          # [G, M, h, w]: chunks of whole groups stay views, read in place
    G, M = int(groups.shape[0]), int(groups.shape[1])
    P, dev, step = G * M, logits.device, max(1, max_planes // M)
    masks = torch.empty((P, oh, ow), dtype=torch.uint8, device=dev)
    changed = torch.empty((P,), dtype=torch.int32, device=dev)
    stats = torch.empty((P, 5), dtype=torch.int32, device=dev)
    for g0 in range(0, G, step):
        raw = ops.mask_binarize(groups[g0:g0 + step], (oh, ow), float(threshold)).reshape(-1, oh, ow)
        p0, p1 = g0 * M, g0 * M + int(raw.shape[0])
        ops.mask_clean(raw, min_area, holes=bool(mode & cc.HOLES), islands=bool(mode & cc.ISLANDS), largest=bool(mode & cc.LARGEST),
                       connectivity=connectivity, out=masks[p0:p1], changed=changed[p0:p1], stats=stats[p0:p1])   # written in place: no copy
    return masks.view(torch.bool).reshape(*lead, oh, ow), changed.reshape(lead), stats.reshape(*lead, 5)


class Segmentation:
    """low_res_logits [B, nb, M, 4g, 4g] fp32 and iou [B, nb, M] fp32 of one decode; M = 1 (mask token 0) or 3 (tokens 1..3)."""

    def __init__(self, low_res_logits: torch.Tensor, iou: torch.Tensor, input_size):
        self.low_res_logits, self.iou, self.input_size = low_res_logits, iou, tuple(int(v) for v in input_size)

    def logits(self, size=None) -> torch.Tensor:
        """Bilinear (align_corners=False) to the input size (S, S) or `size` (h, w): [B, nb, M, h, w] fp32; plain torch."""
        size = self.input_size if size is None else tuple(int(v) for v in size)
        B, nb, M = self.low_res_logits.shape[:3]
        up = torch.nn.functional.interpolate(self.low_res_logits.flatten(0, 1), size=size, mode="bilinear", align_corners=False)
        return up.reshape(B, nb, M, *size)

    def masks(self, size=None, threshold: float = 0.0) -> torch.Tensor:
        return self.logits(size) > threshold

    def stats(self, size=None, threshold: float = 0.0, offset: float = 1.0):
        """(counts int32 [B, nb, M, 3], boxes int32 [B, nb, M, 4], stability fp32 [B, nb, M]) of every mask at the input size or
        `size`: the pixels above threshold + offset, threshold and threshold - offset, the box (min x, min y, max x, max y) of
        those above threshold, and SAM's stability score float(n_hi) / float(n_lo).  ONE vdr.ops.mask_stats call that reads
        low_res_logits in place (tokens 1 .. 3 of the decode's four included); the up-sampled masks are never written."""
        from . import amg, ops
        size = self.input_size if size is None else size
        B, nb, M = (int(v) for v in self.low_res_logits.shape[:3])
        counts, box = ops.mask_stats(self.low_res_logits.flatten(0, 1), size, threshold, offset)
        counts, box = counts.reshape(B, nb, M, 3), box.reshape(B, nb, M, 4)
        return counts, box, amg.stability(counts)

    def clean(self, size=None, threshold: float = 0.0, min_area: int = 0, holes: bool = True, islands: bool = True, largest: bool = False,
              connectivity: int = 8, max_planes: int = 64):
        """(masks bool [B, nb, M, h, w], changed int32 [B, nb, M], stats int32 [B, nb, M, 5]) at the input size or `size`: the masks
        of masks(size, threshold) with holes below min_area filled and islands below it removed (segment_anything's
        remove_small_regions, both passes), or only the largest component kept; changed bit 0 / 1: the hole / island step changed
        the mask; stats: area and inclusive box x0, y0, x1, y1.  One vdr.ops.mask_binarize that reads low_res_logits in place and
        one vdr.ops.mask_clean per chunk of max_planes planes (clean_planes); the binarisation is mask_stats' arithmetic."""
        return clean_planes("Segmentation.clean", self.low_res_logits.flatten(0, 1), self.input_size if size is None else size, threshold, min_area,
                            holes, islands, largest, connectivity, max_planes, lead=tuple(self.low_res_logits.shape[:3]))

    def distance(self, size=None, threshold: float = 0.0) -> torch.Tensor:
        """int32 [B, nb, M, h, w]: the squared Euclidean distance of every mask pixel to the nearest pixel outside its mask (0
        outside the mask, 2^31 - 1 on a mask that fills the plane), at the input size or `size`: ONE vdr.ops.mask_binarize that
        reads low_res_logits in place (the pixels mask_stats counts) and ONE vdr.ops.distance_transform."""
        return distance_planes("Segmentation.distance", self.low_res_logits.flatten(0, 1), self.input_size if size is None else size, threshold,
                               tuple(self.low_res_logits.shape[:3]))

    def inner_points(self):
        """(points fp32 [B, nb, M, 2] (x, y) in pixels of the input, labels int32 [B, nb, M]): the most interior pixel of every
        low-resolution mask (logits > 0; vdr.morphology.inner_point with the plane's outside counted as clear), ready to go
        back in as a positive click; label -1 and point (0, 0) for an empty mask.  No synchronisation."""
        from . import morphology as mo
        lead = tuple(self.low_res_logits.shape[:3])
        pts, lab = mo.inner_point((self.low_res_logits > 0).flatten(0, 2), self.input_size, outside=True)
        return pts.reshape(*lead, 2), lab.reshape(lead)

    def best(self) -> "Segmentation":
        """the highest-IoU mask of every problem (M = 1): a device gather, no synchronisation; ties go to the lowest index"""
        idx = self.iou.argmax(dim=2, keepdim=True)                                  # [B, nb, 1]
        lg = torch.gather(self.low_res_logits, 2, idx[..., None, None].expand(-1, -1, 1, *self.low_res_logits.shape[3:]))
        return Segmentation(lg, torch.gather(self.iou, 2, idx), self.input_size)

    def as_mask_input(self, select="best") -> torch.Tensor:
        """[B, nb, 4g, 4g] fp32: one mask's low-resolution logits per problem, to feed back as `mask_input` (SAM's refinement
        loop).  select: "best" (highest predicted IoU) or the index of a mask."""
        if select == "best":
            return self.best().low_res_logits[:, :, 0]
        if isinstance(select, bool) or not isinstance(select, int) or not 0 <= select < self.low_res_logits.shape[2]:
            raise ValueError(f"as_mask_input: select must be 'best' or an index below {self.low_res_logits.shape[2]}, got {select!r}")
        return self.low_res_logits[:, :, select]


class VolumeSegmentation:
    """What propagate_masks returns: low_res_logits [Z, 4g, 4g] fp32, iou [Z], boxes [Z, 4] fp32 (the box each slice was decoded
    with, in pixels of the prepared input), area [Z] int32 (pixels of the slice's low-resolution mask), all on the device."""

    def __init__(self, low_res_logits, iou, boxes, area, input_size):
        self.low_res_logits, self.iou, self.boxes, self.area = low_res_logits, iou, boxes, area
        self.input_size = tuple(int(v) for v in input_size)

    def logits(self, size=None) -> torch.Tensor:
        size = self.input_size if size is None else tuple(int(v) for v in size)
        return torch.nn.functional.interpolate(self.low_res_logits[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]

    def masks(self, size=None, threshold: float = 0.0) -> torch.Tensor:
        """[Z, h, w] bool at the input size or `size`"""
        return self.logits(size) > threshold

    def clean(self, size=None, threshold: float = 0.0, min_area: int = 0, holes: bool = True, islands: bool = True, largest: bool = False,
              connectivity: int = 8, max_planes: int = 64):
        """(masks bool [Z, h, w], changed int32 [Z], stats int32 [Z, 5]): Segmentation.clean for the slices of a volume, slice by
        slice (2-D components; 3-D ones are out of scope)"""
        return clean_planes("VolumeSegmentation.clean", self.low_res_logits, self.input_size if size is None else size, threshold, min_area, holes,
                            islands, largest, connectivity, max_planes)

    def distance(self, size=None, threshold: float = 0.0, spacing=None) -> torch.Tensor:
        """int32 [Z, h, w]: Segmentation.distance for the slices of a volume, slice by slice (2-D distances).  spacing=(sz, sy, sx),
        the voxel size at `size`: int64 [Z, h, w], the 3-D squared distances of the whole volume in units of the quantum squared
        (vdr.morphology.quantize_spacing; sqrt(d2) * 2^-10 is the distance in spacing's unit)"""
        if spacing is not None:
            from . import morphology as mo
            from . import ops
            what = "VolumeSegmentation.distance"
            q, _ = mo.quantize_spacing(spacing)
            oh, ow = ops.check_out_size(what, self.input_size if size is None else size)
            if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
                raise ValueError(f"{what}: threshold must be a number, got {threshold!r}")
            mo.check_edt3(what, q, 1, False, None, (int(self.low_res_logits.shape[0]), oh, ow))
            return mo._edt3(ops.mask_binarize(self.low_res_logits, (oh, ow), float(threshold)), q, 1, 0)
        return distance_planes("VolumeSegmentation.distance", self.low_res_logits, self.input_size if size is None else size, threshold,
                               (int(self.low_res_logits.shape[0]),))

    def inner_points(self):
        """(points fp32 [Z, 2] (x, y) in pixels of the input, labels int32 [Z]): Segmentation.inner_points slice by slice"""
        from . import morphology as mo
        return mo.inner_point(self.low_res_logits > 0, self.input_size, outside=True)

    def compare(self, other, size=None, threshold: float = 0.0, spacing=1.0, tolerance: float = 1.0) -> dict:
        """This volume's masks against `other` -- another VolumeSegmentation or a bool / uint8 mask tensor [Z, h, w] on the same
        device -- slice by slice at the input size or `size`: vdr.metrics.overlap (dice, iou, intersection, a, b) and
        vdr.metrics.surface (hd, hd95, assd, nsd) in one dict of [Z] tensors.  The distance transforms run on the device; the
        surface measures synchronise once per slice.  spacing=(sz, sy, sx), the voxel size at `size`: the two VOLUMES are compared
        as wholes, in 3-D and in spacing's unit -- every entry is a [1] tensor (vdr.metrics.surface with a 3-sequence)."""
        from . import metrics
        if not isinstance(spacing, (int, float)):
            from . import morphology as mo
            mo.quantize_spacing(spacing)
        size = self.input_size if size is None else tuple(int(v) for v in size)
        a = self.masks(size, threshold)
        b = other.masks(size, threshold) if isinstance(other, VolumeSegmentation) else other
        if not isinstance(b, torch.Tensor) or tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"VolumeSegmentation.compare: other must be a VolumeSegmentation or a mask tensor {tuple(a.shape)}, got "
                             f"{tuple(b.shape) if isinstance(b, torch.Tensor) else type(b).__name__}")
        if not isinstance(spacing, (int, float)):
            out = metrics.overlap(a, b, volumes=True)
            out.update(metrics.surface(a, b, spacing=spacing, tolerance=tolerance))
            return out
        out = metrics.overlap(a, b)
        out.update(metrics.surface(a, b, spacing=spacing, tolerance=tolerance))
        return out


def distance_planes(what: str, logits, size, threshold, lead):
    """planes of low-resolution logits [P, h, w] or [G, M, h, w] on the device -> d2 int32 [*lead, oh, ow] of their masks at `size`"""
    from . import ops
    oh, ow = ops.check_out_size(what, size)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError(f"{what}: threshold must be a number, got {threshold!r}")
    raw = ops.mask_binarize(logits, (oh, ow), float(threshold)).reshape(-1, oh, ow)
    return ops.distance_transform(raw).reshape(*lead, oh, ow)


MAX_TOKENS = 16                     # per problem (include/vdr.h): 5 + points + (2 with a box, 1 without)
POINT_LABELS = (1, 0, -1, -10)      # foreground, background, not a point, transformers' padding


def _real(what, name, t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor or array, got {type(t).__name__}")
    if t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"{what}: {name} must hold real numbers, got {t.dtype}")
    return t


def check_prompts(what: str, boxes, points, labels, mask_input, batch, g=None, decoder=None):
    """Every prompt of one decode, before any device work -> (boxes, points, labels, mask_input) as tensors or None.  points
    [B, nb, np, 2] (x, y) with labels [B, nb, np]; mask_input [B, nb, 4g, 4g] or [B, 1, 4g, 4g] / [B, 4g, 4g] (one per image)."""
    if boxes is None and points is None:
        raise ValueError(f"{what}: no prompt: give boxes, points or both")
    if boxes is not None:
        boxes = check_boxes(what, boxes, batch)
    nb = None if boxes is None else int(boxes.shape[1])
    if (points is None) != (labels is None):
        raise ValueError(f"{what}: points and point_labels go together")
    if points is not None:
        points, labels = _real(what, "points", points), _real(what, "point_labels", labels)
        if points.dim() != 4 or points.shape[-1] != 2 or points.shape[1] < 1 or points.shape[2] < 1:
            raise ValueError(f"{what}: points must be [B, nb, np, 2] (x, y), got {tuple(points.shape)}")
        if tuple(labels.shape) != tuple(points.shape[:3]):
            raise ValueError(f"{what}: point_labels must be {tuple(points.shape[:3])}, got {tuple(labels.shape)}")
        if labels.is_floating_point():
            raise ValueError(f"{what}: point_labels must be integers, got {labels.dtype}")
        if batch is not None and points.shape[0] != batch:
            raise ValueError(f"{what}: {points.shape[0]} point sets for {batch} images")
        if nb is not None and points.shape[1] != nb:
            raise ValueError(f"{what}: nb mismatch: {nb} boxes per image, {points.shape[1]} point sets per image")
        nb = int(points.shape[1])
        T = 5 + int(points.shape[2]) + (2 if boxes is not None else 1)
        if T > MAX_TOKENS:
            raise ValueError(f"{what}: {T} tokens per problem (5 + {points.shape[2]} points + {2 if boxes is not None else 1}); at most {MAX_TOKENS}")
        if not labels.is_cuda and not bool(torch.isin(labels, torch.tensor(POINT_LABELS, dtype=labels.dtype)).all()):
            raise ValueError(f"{what}: point_labels must be 1 (foreground), 0 (background), -1 (not a point) or -10 (padding)")
    if decoder is not None and (points is not None or boxes is None) and not decoder.has_point_prompts:
        raise ValueError(f"{what}: the checkpoint has no point-prompt weights (point_embeddings.0/1, not_a_point_embed): weights absent")
    if mask_input is not None:
        mask_input = _real(what, "mask_input", mask_input)
        B = int(points.shape[0] if boxes is None else boxes.shape[0])
        ok = mask_input.is_floating_point() and mask_input.dim() in (3, 4) and mask_input.shape[0] == B
        if ok and g is not None:
            ok = tuple(mask_input.shape[-2:]) == (4 * g, 4 * g)
        if ok and mask_input.dim() == 4:
            ok = mask_input.shape[1] in (1, nb)
        if not ok:
            side = "4g" if g is None else str(4 * g)
            raise ValueError(f"{what}: wrong mask shape: mask_input must be floating [{B}, {nb}, {side}, {side}], or [{B}, 1, {side}, {side}] / "
                             f"[{B}, {side}, {side}] (one per image), got {tuple(mask_input.shape)} {mask_input.dtype}")
        if decoder is not None and not decoder.has_mask_prompt:
            raise ValueError(f"{what}: the checkpoint has no mask-prompt weights (prompt_encoder.mask_downscaling.*): weights absent")
    return boxes, points, labels, mask_input


def check_boxes(what: str, boxes, batch=None) -> torch.Tensor:
    """boxes [B, nb, 4] (x0, y0, x1, y1) of a real dtype, before any device work"""
    if isinstance(boxes, np.ndarray):
        boxes = torch.from_numpy(boxes)
    if not isinstance(boxes, torch.Tensor):
        raise ValueError(f"{what}: boxes must be a tensor or array [B, nb, 4], got {type(boxes).__name__}")
    if boxes.dim() != 3 or boxes.shape[-1] != 4 or boxes.shape[1] < 1:
        raise ValueError(f"{what}: boxes must be [B, nb, 4] (x0, y0, x1, y1), got {tuple(boxes.shape)}")
    if boxes.dtype == torch.bool or boxes.is_complex() or not (boxes.is_floating_point() or boxes.dtype in (
            torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
        raise ValueError(f"{what}: boxes must hold real numbers, got {boxes.dtype}")
    if batch is not None and boxes.shape[0] != batch:
        raise ValueError(f"{what}: {boxes.shape[0]} box sets for {batch} images")
    return boxes


def fourier_pe(coords01: torch.Tensor, gauss: torch.Tensor) -> torch.Tensor:
    """[..., 2] (x, y) in [0, 1] -> [..., 2 * gauss.shape[1]] float64: cat(sin, cos)(2 pi (2c - 1) G)"""
    c = (2.0 * coords01.double() - 1.0) @ gauss.double()
    c = 2.0 * math.pi * c
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


class MaskDecoder:
    """The decoder object of one SAM handle at one grid: a vdr_mask_decoder handle of libvdr (include/vdr.h).  weights:
    segment_anything-spelled tensors (vdr.weights.split_sam_decoder_weights); the library rounds the GEMM weights to bf16, stacks
    the projections and builds the positional-encoding tables once, in vdr_mask_decoder_finalize."""

    LAUNCHES = 52   # of one decode, whatever B and nb: 2 of set-up (tokens, keys) + 18 per block + 5 + 3 + 3 + 3 (include/vdr.h)

    def __init__(self, weights, grid: int, img: int, device, ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6):
        import ctypes as C
        self.g, self.img, self.device = int(grid), int(img), torch.device(device)
        lin1 = weights.get("mask_decoder.transformer.layers.0.mlp.lin1.weight")
        if lin1 is None or "mask_decoder.transformer.layers.1.cross_attn_image_to_token.out_proj.weight" not in weights:
            raise ValueError("mask decoder: the weights of a two-layer TwoWayTransformer are expected")
        self.mlp_dim = int(lin1.shape[0])
        self.lib = L.load()
        cfg = L.vdr_mask_decoder_config(grid=self.g, img=self.img, channels=256, heads=8, depth=2, mlp_dim=self.mlp_dim,
                                        attention_downsample_rate=2, mask_tokens=4, upscale_channels_1=64, upscale_channels_2=32,
                                        iou_head_depth=3, ln_eps=float(ln_eps), final_ln_eps=float(final_ln_eps), ln2d_eps=float(ln2d_eps))
        h = C.c_void_p()
        L.check(self.lib.vdr_mask_decoder_create(C.byref(cfg), self.device.index or 0, C.byref(h)))
        self.h = h

        def set_weight(name):
            t = torch.as_tensor(weights[name]).detach().to(torch.float32).contiguous().cpu()
            shape = (C.c_int64 * t.dim())(*t.shape)
            L.check(self.lib.vdr_mask_decoder_set_weight(h, name.encode(), t.data_ptr(), shape, t.dim()))

        for i in range(self.lib.vdr_mask_decoder_num_weights(h)):
            name = self.lib.vdr_mask_decoder_weight_name(h, i).decode()
            if name not in weights:
                raise ValueError(f"mask decoder: the checkpoint has no {name}")
            set_weight(name)
        # the optional prompt weights: a group is set when the checkpoint holds all of it
        opt = [self.lib.vdr_mask_decoder_prompt_weight_name(h, i).decode() for i in range(self.lib.vdr_mask_decoder_num_prompt_weights(h))]
        for group in (opt[:3], opt[3:]):
            if all(n in weights for n in group):
                for name in group:
                    set_weight(name)
        L.check(self.lib.vdr_mask_decoder_finalize(h))
        support = self.lib.vdr_mask_decoder_prompt_support(h)
        self.has_point_prompts, self.has_mask_prompt = bool(support & L.PROMPT_POINTS), bool(support & L.PROMPT_MASK)

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.vdr_mask_decoder_destroy(h)

    def workspace_bytes(self, problems: int, tokens: int = 7) -> int:
        import ctypes as C
        n = C.c_size_t()
        if tokens == 7:
            L.check(self.lib.vdr_mask_decoder_workspace_bytes(self.h, int(problems), C.byref(n)))
        else:
            L.check(self.lib.vdr_mask_decoder_workspace_bytes_prompts(self.h, int(problems), int(tokens), C.byref(n)))
        return int(n.value)

    def decode(self, emb: torch.Tensor, boxes=None, points=None, labels=None, mask_input=None, workspace=None):
        """emb [B, 256, g, g] on the device (a channel-first view of the encoder's [B, g, g, 256] output is read in place), boxes
        [B, nb, 4] and / or points [B, nb, np, 2] with labels [B, nb, np], mask_input [B, nb, 4g, 4g] or one per image ([B, 1, 4g, 4g]
        / [B, 4g, 4g]) -> (low_res_logits [B, nb, 4, 4g, 4g] fp32, iou [B, nb, 4] fp32) of all four mask tokens: ONE vdr_mask_decode
        (boxes alone) or vdr_mask_decode_prompts call on the current stream.  workspace: a uint8 device tensor of at least
        workspace_bytes(B * nb, tokens), else allocated here."""
        import ctypes as C
        boxes, points, labels, mask_input = check_prompts("decode", boxes, points, labels, mask_input, int(emb.shape[0]), self.g, self)
        lead = boxes if boxes is not None else points
        B, nb = int(lead.shape[0]), int(lead.shape[1])
        P = B * nb
        npts = 0 if points is None else int(points.shape[2])
        T = 5 + npts + (2 if boxes is not None else 1)
        emb = emb.to(self.device, torch.float32)
        if emb.permute(0, 2, 3, 1).is_contiguous():
            channels_last = 1
        else:
            emb, channels_last = emb.contiguous(), 0
        bx = None if boxes is None else boxes.to(self.device, torch.float32).contiguous()
        need = self.workspace_bytes(P, T)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        logits = torch.empty((B, nb, 4, 4 * self.g, 4 * self.g), dtype=torch.float32, device=self.device)
        iou = torch.empty((B, nb, 4), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if points is None and mask_input is None:
            L.check(self.lib.vdr_mask_decode(self.h, emb.data_ptr(), channels_last, bx.data_ptr(), B, nb, workspace.data_ptr(), workspace.numel(),
                                             logits.data_ptr(), iou.data_ptr(), stream))
            return logits, iou
        pr = L.vdr_mask_prompts(boxes=None if bx is None else bx.data_ptr())
        if points is not None:
            pt = points.to(self.device, torch.float32).contiguous()
            lb = labels.to(self.device, torch.int32).contiguous()
            pr.points, pr.labels, pr.points_per_problem = pt.data_ptr(), lb.data_ptr(), npts
        if mask_input is not None:
            mk = mask_input.to(self.device, torch.float32)
            per_image = mk.dim() == 3 or (mk.shape[1] == 1 and nb != 1)
            mk = mk.reshape(-1, 4 * self.g, 4 * self.g).contiguous()
            pr.mask_input, pr.mask_per_image = mk.data_ptr(), int(per_image)
        L.check(self.lib.vdr_mask_decode_prompts(self.h, emb.data_ptr(), channels_last, C.byref(pr), B, nb, workspace.data_ptr(), workspace.numel(),
                                                 logits.data_ptr(), iou.data_ptr(), stream))
        return logits, iou


def select_masks(logits, iou, multimask: bool):
    """mask token 0 (multimask=False) or tokens 1..3 of one decode's four"""
    return (logits[:, :, 1:], iou[:, :, 1:]) if multimask else (logits[:, :, :1], iou[:, :, :1])


def scale_box(box, h: int, w: int, side: int) -> "tuple[float, float, float, float]":
    """(x0, y0, x1, y1) in pixels of an (h, w) slice -> pixels of the side x side prepared image (prepare_image's resize)"""
    x0, y0, x1, y1 = (float(v) for v in box)
    sx, sy = side / float(w), side / float(h)
    return (x0 * sx, y0 * sy, x1 * sx, y1 * sy)


def _require(model, what):
    cfg = getattr(model, "cfg", None)
    if cfg is None or getattr(cfg, "window", 0) <= 0:
        raise ValueError(f"{what}: prompted segmentation needs a SAM / MedSAM model, got '{getattr(model, 'model_name', type(model).__name__)}'")
    if not getattr(model, "has_mask_decoder", False):
        raise ValueError(f"{what}: the model was loaded without prompt_encoder.* / mask_decoder.* weights (an encoder-only checkpoint)")


def segment_slice(model, img, box=None, multimask: bool = False, threshold: float = 0.0, points=None, point_labels=None) -> np.ndarray:
    """get_dense_descriptor's sibling: a RAW (h, w) gray or (h, w, 3) colour slice in [0, 1] and one box (x0, y0, x1, y1) in slice
    pixels and / or points [np, 2] (x, y) in slice pixels with point_labels [np] -> the (h, w) bool mask at slice resolution
    ((M, h, w) with multimask).  The slice is prepared as prepare_image does, the box and the points scaled by the same factors."""
    from . import prep
    _require(model, "segment_slice")
    t = torch.as_tensor(img)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
        raise ValueError(f"segment_slice: a raw (h, w) / (h, w, 3) slice, got {tuple(t.shape)}")
    h, w = int(t.shape[0]), int(t.shape[1])
    side = model.cfg.img
    boxes = pts = lbl = None
    if box is not None:
        b = torch.as_tensor(box)
        if b.shape != (4,):
            raise ValueError(f"segment_slice: box must be (x0, y0, x1, y1), got {tuple(b.shape)}")
        check_boxes("segment_slice", b.reshape(1, 1, 4))
        boxes = torch.tensor([[scale_box(b.tolist(), h, w, side)]], dtype=torch.float64)
    if points is not None or point_labels is not None:
        if points is None or point_labels is None:
            raise ValueError("segment_slice: points and point_labels go together")
        p, lbl = torch.as_tensor(points), torch.as_tensor(point_labels)
        if p.dim() != 2 or p.shape[1] != 2 or tuple(lbl.shape) != (p.shape[0],):
            raise ValueError(f"segment_slice: points must be [np, 2] (x, y) with point_labels [np], got {tuple(p.shape)} and {tuple(lbl.shape)}")
        pts = (p.double() * torch.tensor([side / float(w), side / float(h)], dtype=torch.float64))[None, None]
        lbl = lbl[None, None]
    check_prompts("segment_slice", boxes, pts, lbl, None, 1, decoder=model.mask_decoder)
    x = prep.prepare_image(t, side=side, device=model.device)
    m = model.segment(x, boxes, points=pts, point_labels=lbl, multimask=multimask).masks(size=(h, w), threshold=threshold)[0, 0]
    return (m if multimask else m[0]).cpu().numpy()
