"""Host-side mirror of the reference's call boundary for the hot path.

    R1  load_model(model_name, model_path)              src/tfds_dense_descriptor.py:51-67
    R2  model.image_encoder(x) / model.patch_embed(x)   src/tfds_dense_descriptor.py:122-129
        get_dense_descriptor(model, img) -> (h, w, D)   src/tfds_dense_descriptor.py:110-139
    R3  model(x[B,S,D]) -> (logits[B,C], cls[B,D])      src/models_archs.py:141-147

Same names, argument meaning and error behaviour (Python exceptions); everything below these
methods runs in libvdr.so on the MI355X.  There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .engine import (AttnMap, Engine, FacetOut, LayerOut, VdrConfig, check_descriptor_model, check_facet, check_input_size,
                     check_patch_stride)

_DINOV3 = dict(layerscale=True, has_pos=False, ln_eps=1e-5, n_register=4, rope=True, rope_theta=100.0)

# geometries BASELINE.json names + the two the reference itself loads
ARCHS = {
    "vit_tiny16_224": VdrConfig(224, 16, 3, 192, 3, 12, 768),
    "vit_base16_224": VdrConfig(224, 16, 3, 768, 12, 12, 3072),
    "vit_large14_336": VdrConfig(336, 14, 3, 1024, 16, 24, 4096),
    "dinov2_giant14_224": VdrConfig(224, 14, 3, 1536, 24, 40, 4096, act="swiglu", layerscale=True),
    # reference default for model_name='dinov2': load_dinov2('small') = dinov2_vits14, of which the hot loop runs
    # `model.patch_embed(x)` ONLY, at 896x896 (tfds_dense_descriptor.py:128-133).  So the drop-in for that name is the
    # patch embedding alone: no blocks, no cls / pos / norm -- a real dinov2_vits14 state_dict loads as it is (its
    # pos_embed [1, 1370, 384] for 518^2, cls_token / mask_token / blocks.* / norm.* keys are ignored here exactly as
    # the reference ignores them; the whole encoder of that checkpoint is "dinov2_small14_518" below).
    "dinov2": VdrConfig(896, 14, 3, 384, 6, 0, 1536, pre_ln=False, has_cls=False, has_pos=False),
    # the whole ViT-S/14 with a table native to 896^2 (pos_embed [1, 4097, 384]: a checkpoint resized beforehand; it
    # runs at 896^2 on the loaded table itself and at any other size through set_input_size)
    "dinov2_small14_896": VdrConfig(896, 14, 3, 384, 6, 12, 1536, layerscale=True),
    # the whole ViT-S/14 at its pre-training size: a real dinov2_vits14 state_dict (pos_embed [1, 1370, 384]) loads as it
    # is and runs at 224^2, 896^2, ... after set_input_size / with dynamic_size=True (DINOv2's interpolate_pos_encoding)
    "dinov2_small14_518": VdrConfig(518, 14, 3, 384, 6, 12, 1536, layerscale=True),
    # reference default backbone: sam_model_registry['vit_b'] image encoder (MedSAM checkpoint), 1024x1024
    "medsam": VdrConfig(1024, 16, 3, 768, 12, 12, 3072, has_cls=False, window=14, global_blocks=(2, 5, 8, 11),
                        neck_chans=256),
    # vision towers of language-supervised models (transformers CLIPVisionModel[WithProjection] / SiglipVisionModel).
    # OpenAI CLIP and its medical descendants (PubMedCLIP, QuiltNet, PLIP): QuickGELU, pre_layrnorm (input_ln), eps 1e-5
    "clip_vit_base16_224": VdrConfig(224, 16, 3, 768, 12, 12, 3072, act="quick_gelu", input_ln=True, ln_eps=1e-5),
    "clip_vit_base32_224": VdrConfig(224, 32, 3, 768, 12, 12, 3072, act="quick_gelu", input_ln=True, ln_eps=1e-5),
    "clip_vit_large14_336": VdrConfig(336, 14, 3, 1024, 16, 24, 4096, act="quick_gelu", input_ln=True, ln_eps=1e-5),
    # SigLIP (siglip-base / large-patch16): tanh-GELU, no CLS token, attention-pooling head, eps 1e-6
    "siglip_base16_224": VdrConfig(224, 16, 3, 768, 12, 12, 3072, act="gelu_tanh", has_cls=False),
    "siglip_large16_256": VdrConfig(256, 16, 3, 1024, 16, 24, 4096, act="gelu_tanh", has_cls=False),
    # DINOv2-with-registers (hub dinov2_vit*14_reg / transformers Dinov2WithRegistersModel): DINOv2 plus 4 register tokens
    # between the CLS row and the patch rows; pos_embed [1, 1370, D] for 518^2, other sizes through set_input_size
    "dinov2_small14_reg_518": VdrConfig(518, 14, 3, 384, 6, 12, 1536, layerscale=True, n_register=4),
    "dinov2_base14_reg_518": VdrConfig(518, 14, 3, 768, 12, 12, 3072, layerscale=True, n_register=4),
    "dinov2_large14_reg_518": VdrConfig(518, 14, 3, 1024, 16, 24, 4096, layerscale=True, n_register=4),
    "dinov2_giant14_reg_518": VdrConfig(518, 14, 3, 1536, 24, 40, 4096, act="swiglu", layerscale=True, n_register=4),
    # DINOv3 (transformers DINOv3ViTModel): 4 register tokens, no pos_embed, 2-D RoPE on q / k of the patch rows,
    # LayerScale, eps 1e-5; the "plus" models have the gated (SwiGLU) MLP
    "dinov3_vits16": VdrConfig(224, 16, 3, 384, 6, 12, 1536, **_DINOV3),
    "dinov3_vits16plus": VdrConfig(224, 16, 3, 384, 6, 12, 1536, act="swiglu", **_DINOV3),
    "dinov3_vitb16": VdrConfig(224, 16, 3, 768, 12, 12, 3072, **_DINOV3),
    "dinov3_vitl16": VdrConfig(224, 16, 3, 1024, 16, 24, 4096, **_DINOV3),
    "dinov3_vith16plus": VdrConfig(224, 16, 3, 1280, 20, 32, 5120, act="swiglu", **_DINOV3),
}


def from_sam_state_dict(sd):
    """segment_anything checkpoint keys (image_encoder.* of sam_model_registry['vit_b'](path),
    tfds_dense_descriptor.py:104) -> the canonical names vdr_set_weight understands."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("image_encoder."):
            continue
        k = k[len("image_encoder."):].replace(".mlp.lin1.", ".mlp.fc1.").replace(".mlp.lin2.", ".mlp.fc2.")
        out[k] = v
    return out


def sam_input_side(img_size, patch: int) -> int:
    """The square input side a SAM encoder is built at (load_model's img_size): one int, or an equal (h, w) pair; a
    positive multiple of the patch side with at most 64 patches a side (the global-attention kernels' limit)."""
    if isinstance(img_size, (tuple, list)):
        if len(img_size) != 2 or int(img_size[0]) != int(img_size[1]):
            raise ValueError(f"img_size: the SAM encoder takes square inputs, got {tuple(img_size)}")
        img_size = img_size[0]
    side = int(img_size)
    if side <= 0 or side % patch:
        raise ValueError(f"img_size must be a positive multiple of the patch side {patch}, got {side}")
    if side // patch > 64:
        raise ValueError(f"img_size {side}: {side // patch} patches a side, the SAM global attention takes at most 64")
    return side


def block_indices(idx, depth: int, what: str) -> "list[int]":
    """A sequence of block indices as ints, in the order given; an empty one or an index outside 0..depth-1: ValueError."""
    idx = [int(i) for i in idx]
    if not idx:
        raise ValueError(f"{what}: no block index given")
    bad = [i for i in idx if not 0 <= i < depth]
    if bad:
        raise ValueError(f"block indices {bad} out of range 0..{depth - 1}")
    return idx


def check_batch(what: str, x) -> None:
    """The one wording of "x is no image batch" (ValueError); the size is the engine's to check."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{what}: x must be [B, 3, H, W], got {tuple(getattr(x, 'shape', ()))}")


def facet_args(model, what: str, layer, facet, bin, hierarchy, sentence: str) -> int:
    """The descriptor arguments of a method that also takes facet=None (the model's own dense descriptor, which has no block to
    choose and nothing to bin: a layer or bin is refused with `sentence`); a facet: model._descriptor_args' refusals.  Returns the
    hierarchy to ask for."""
    if facet is not None:
        return model._descriptor_args(layer, facet, bool(bin), False, hierarchy)
    if layer is not None or bin:
        raise ValueError(f"{what}: {sentence}")
    return 0


def intermediate_layer_indices(n, depth: int) -> "list[int]":
    """The blocks DINOv2's get_intermediate_layers returns (DinoVisionTransformer._get_intermediate_layers_not_chunked):
    an int n means the last n blocks; a sequence means those block indices, returned in block order (the blocks are
    visited in order and kept when listed), each once.  Anything DINOv2 would fail on is a ValueError here."""
    if isinstance(n, bool):
        raise ValueError("n must be an int or a sequence of block indices")
    if isinstance(n, (int, np.integer)):
        if not 1 <= int(n) <= depth:
            raise ValueError(f"n = {n}: the model has {depth} blocks")
        return list(range(depth - int(n), depth))
    idx = block_indices(n, depth, "n")
    if len(set(idx)) != len(idx):
        raise ValueError(f"block indices {idx} repeat one")
    return sorted(idx)


@dataclass
class Correspondences:
    """Result of VitDescriptorModel.find_correspondences for B image pairs on a gh x gw grid of t = gh * gw patches.
    nn12 [B, t] int32: for every patch of image 1 its cosine-nearest patch of image 2, sim12 [B, t] fp32 that similarity;
    nn21 / sim21 the reverse.  saliency1 / saliency2 [B, t] fp32: the last block's CLS attention over the patch columns,
    mean over the heads, min-max normalised per image.  mask [B, t] bool: best buddies (nn21[nn12[i]] == i) whose two
    patches are both salient (> thresh).  grid = (gh, gw); stride and patch place a grid index in the image.
    desc1 / desc2 [B, t, d] bf16: the descriptors that were matched, kept with find_correspondences(keep_descriptors=True)
    (None otherwise); points(select="kmeans") needs them.
    radius: None for the global match; r for find_correspondences(radius=r), where both directions were searched inside the
    (2r + 1) x (2r + 1) window around every patch's own grid position (vdr.ops.local_correlation).  cost12 [B, t, (2r + 1)^2]
    fp32: the cost volume of the 1 -> 2 direction, kept with keep_cost=True (None otherwise); vdr.local.topk and
    vdr.local.soft_displacement take it."""
    nn12: torch.Tensor
    sim12: torch.Tensor
    nn21: torch.Tensor
    sim21: torch.Tensor
    saliency1: torch.Tensor
    saliency2: torch.Tensor
    mask: torch.Tensor
    grid: "tuple[int, int]"
    stride: int
    patch: int
    desc1: torch.Tensor = None
    desc2: torch.Tensor = None
    # (set by find_correspondences; plain attributes, not dataclass fields: the constructor and the field list stay what they were)
    radius = None
    cost12 = None

    def displacement(self) -> torch.Tensor:
        """[B, gh, gw, 2] int32: how far every patch of image 1 moved to its match nn12 in image 2, (dy, dx) in patches"""
        gh, gw = self.grid
        i = torch.arange(gh * gw, device=self.nn12.device).unsqueeze(0)
        j = self.nn12.long()
        dy = torch.div(j, gw, rounding_mode="floor") - torch.div(i, gw, rounding_mode="floor")
        return torch.stack((dy, j % gw - i % gw), dim=-1).to(torch.int32).reshape(-1, gh, gw, 2)

    def pixel_displacement(self) -> torch.Tensor:
        """displacement() in pixels: times the patch stride"""
        return self.displacement() * int(self.stride)

    def buddy_descriptors(self, b: int):
        """(positions [n_bb] of the masked buddies of pair b in image 1, ascending; their [n_bb, 2d] bf16 descriptors: the
        L2-normalised (fp32, norm clamped at 1e-12) descriptor of the patch and of its buddy, each rounded once to bf16,
        side by side)"""
        if self.desc1 is None or self.desc2 is None:
            raise ValueError("Correspondences: the descriptors were not kept; call find_correspondences(keep_descriptors=True)")
        idx = torch.nonzero(self.mask[b], as_tuple=False).flatten()
        d1 = self.desc1[b][idx].float()
        d2 = self.desc2[b][self.nn12[b][idx].long()].float()
        norm = torch.nn.functional.normalize
        return idx, torch.cat([norm(d1, dim=-1, eps=1e-12).to(torch.bfloat16), norm(d2, dim=-1, eps=1e-12).to(torch.bfloat16)], dim=-1)

    def points(self, b: int, num_pairs=None, select: str = "similarity"):
        """The correspondences of pair b as two [k, 2] float tensors of (y, x) pixel centres (image 1, image 2), patch
        (gy, gx) at gy * stride + patch / 2.
        select="similarity": the masked positions in order of descending sim12 (ties: ascending position), cut to num_pairs.
        select="kmeans" (dino-vit-features' selection; needs num_pairs and the kept descriptors): the masked buddies'
        descriptors (buddy_descriptors) are clustered by vdr.kmeans.fit(k=min(num_pairs, n_bb), init="maximin"); from every
        non-empty cluster the buddy with the largest rank saliency1 * saliency2[nn12] is taken (lowest position on a tie),
        and the chosen ones come in descending order of that rank (ties: ascending position)."""
        if select not in ("similarity", "kmeans"):
            raise ValueError(f"points: select must be 'similarity' or 'kmeans', got {select!r}")
        if select == "kmeans":
            if num_pairs is None or int(num_pairs) < 1:
                raise ValueError("points: select='kmeans' needs num_pairs >= 1")
            idx, desc = self.buddy_descriptors(b)
            if idx.numel():
                from . import kmeans
                k = min(int(num_pairs), int(idx.numel()), 1024)
                labels = kmeans.fit(desc, k, init="maximin").labels[0]
                rank = self.saliency1[b][idx] * self.saliency2[b][self.nn12[b][idx].long()]
                idx = idx[select_by_cluster(labels, rank, k)]
        else:
            idx = torch.nonzero(self.mask[b], as_tuple=False).flatten()
            order = torch.sort(self.sim12[b][idx], descending=True, stable=True).indices
            idx = idx[order]
            if num_pairs is not None:
                idx = idx[: int(num_pairs)]
        gw = self.grid[1]

        def centres(i):
            i = i.long()
            y, x = torch.div(i, gw, rounding_mode="floor"), i % gw
            return torch.stack((y, x), dim=1).float() * self.stride + self.patch / 2

        return centres(idx), centres(self.nn12[b][idx])


def select_by_cluster(labels: torch.Tensor, rank: torch.Tensor, k: int) -> torch.Tensor:
    """labels [n] in 0..k-1, rank [n] -> the positions (int64) of the top-ranked member of every non-empty cluster, the lowest
    position on a tie, in descending order of rank (ties: ascending position).  Pure torch; CPU tensors work too."""
    n = labels.shape[0]
    pos = torch.arange(n, device=labels.device)
    member = labels.long().unsqueeze(0) == torch.arange(k, device=labels.device).unsqueeze(1)  # [k, n]
    best = torch.where(member, rank.unsqueeze(0), torch.full_like(rank, float("-inf")).unsqueeze(0)).max(dim=1, keepdim=True).values
    first = torch.where(member & (rank.unsqueeze(0) == best), pos, n).min(dim=1).values
    chosen = first[first < n]
    chosen = chosen.sort().values
    return chosen[torch.sort(rank[chosen], descending=True, stable=True).indices]


@dataclass
class Propagation:
    """Result of VitDescriptorModel.propagate_labels for B (source, target) slice pairs on a gh x gw grid.  scores
    [B, gh, gw, n_classes] fp32: every target patch's class scores, the softmax-weighted vote of its k best source patches
    inside the window (they sum to 1); labels [B, gh, gw] int64: the class of the largest score, the lowest on a tie;
    idx [B, t, k] int32 / val [B, t, k] fp32: those source patches and their similarities, best first.  radius is None when
    the search was global (transfer_labels)."""
    scores: torch.Tensor
    labels: torch.Tensor
    idx: torch.Tensor
    val: torch.Tensor
    grid: "tuple[int, int]"
    radius: int


@dataclass
class VolumePropagation:
    """Result of VitDescriptorModel.propagate_volume for the Z slices of a volume on a gh x gw grid.  scores [Z, gh, gw, C]
    fp32: every patch's soft class scores (slice `index`: what was given, a hard map as one-hot; a propagated slice: rows that
    sum to 1 up to rounding); labels [Z, gh, gw] int64: the class of the largest score, the lowest on a tie.  A slice the sweep
    did not visit (below `index` with direction="up", above it with "down") has scores 0 and labels -1.  grid = (gh, gw);
    stride and patch place a grid index in the image."""
    scores: torch.Tensor
    labels: torch.Tensor
    grid: "tuple[int, int]"
    radius: int
    index: int
    stride: int
    patch: int

    def upsample_guided(self, x: torch.Tensor, box=None, **kwargs) -> torch.Tensor:
        """The labels at pixel resolution, [Z, h, w] int64 over `box` (None: the whole image): the soft scores through
        vdr.upsample.guided with the slices x [Z, 3, H, W] themselves as the guide (fp32 out; kwargs: its radius and sigmas),
        then the lowest arg-max.  An unvisited slice comes out as class 0."""
        from . import knn, upsample
        guide = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
        up = upsample.guided(self.scores, guide.to(self.scores.device), self.patch, self.stride, box=box, out_dtype=torch.float32,
                             **kwargs)
        return knn.lowest_argmax(up)


@dataclass
class Cosegmentation:
    """Result of VitDescriptorModel.cosegment for B images on a gh x gw grid.  labels [B, gh, gw] int32: every patch's cluster
    of the one joint k-means over all B maps; salient [k] bool: the clusters voted salient; masks [B, gh, gw] bool: the
    patches in a salient cluster; saliency [B, gh, gw] fp32: the last block's CLS attention, head mean, min-max normalised
    per image; kmeans: the fit (vdr.kmeans.KMeans, one problem)."""
    labels: torch.Tensor
    salient: torch.Tensor
    masks: torch.Tensor
    saliency: torch.Tensor
    kmeans: object


def minmax_normalise(a: torch.Tensor) -> torch.Tensor:
    """(a - min) / (max - min) over the last dimension (a constant row gives zeros)"""
    lo, hi = a.min(dim=-1, keepdim=True).values, a.max(dim=-1, keepdim=True).values
    return (a - lo) / (hi - lo).clamp_min(torch.finfo(a.dtype).tiny)


class VitDescriptorModel:
    """Frozen-ViT feature extractor with the attributes the reference's hot loop dispatches on."""

    def __init__(self, cfg: VdrConfig, weights: "dict[str, torch.Tensor]", model_name: str = "vit", device=None,
                 dynamic_size: bool = False, sized: bool = False, decoder_weights=None, decoder_eps=None):
        """decoder_weights (SAM models): the checkpoint's prompt_encoder.* / mask_decoder.* tensors under their segment_anything
        names (vdr.weights.split_sam_decoder_weights) -- the handle then segments: segment / decode_masks (vdr/segment.py).
        decoder_eps: the three LayerNorm eps of the decoder (vdr.segment.SA_EPS by default, HF_EPS for transformers' values).
        sized=True (SAM encoders built at another side than the reference's 1024, load_model's img_size):
        get_dense_descriptor prepares a raw slice at cfg.img in one resize.  dynamic_size=True: every image method first adopts the size of the images it is given (x.shape[-2:]), as
        DINOv2 and transformers do with interpolate_pos_encoding; the position table is rebuilt only when the size
        changes.  False (default): other sizes are refused until set_input_size names one."""
        if dynamic_size and cfg.window > 0:
            raise ValueError("dynamic_size: the SAM encoder's position tables and window partition are tied to its "
                             f"{cfg.img}x{cfg.img} input")
        self.cfg = cfg
        self.model_name = model_name  # tfds_dense_descriptor.py:66 assigns this attribute
        self.dynamic_size = bool(dynamic_size)
        self.sized = bool(sized)
        self.engine = Engine(cfg, device)
        # (head.* entries -- a translated CLIP projection / SigLIP pooling head -- are not weights of the encoder)
        from .weights import split_head_weights
        weights, head = split_head_weights(weights)
        self.engine.load_weights(weights)
        self.device = self.engine.device
        self.head = None
        if "head.visual_projection.weight" in head:
            self.head = _ClipProjection(head, self.device)
        elif "head.probe" in head:
            self.head = _SiglipPoolHead(head, cfg, self.device)
        self.mask_decoder = None
        if decoder_weights is not None:
            if cfg.window <= 0:
                raise ValueError("decoder_weights: the mask decoder belongs to SAM / MedSAM models")
            from .segment import SA_EPS, MaskDecoder
            self.mask_decoder = MaskDecoder(decoder_weights, cfg.img // cfg.patch, cfg.img, self.device, **(decoder_eps or SA_EPS))

    # -- prompt -> mask (SAM / MedSAM with decoder weights; vdr/segment.py) ----------------------
    @property
    def has_mask_decoder(self) -> bool:
        return getattr(self, "mask_decoder", None) is not None

    def decode_masks(self, emb: torch.Tensor, boxes=None, points=None, point_labels=None, mask_input=None, multimask: bool = False):
        """The prompt encoder and mask decoder alone, on an embedding the caller holds: emb [B, 256, g, g] (what image_encoder
        returns), boxes [B, nb, 4] (x0, y0, x1, y1) and / or points [B, nb, np, 2] (x, y) with point_labels [B, nb, np] (1 foreground,
        0 background, -1 not a point, -10 padding), all in pixels of the input image; mask_input [B, nb, 4g, 4g] (or one per image:
        [B, 1, 4g, 4g] / [B, 4g, 4g]), a decode's own low-resolution logits (Segmentation.as_mask_input) -> vdr.Segmentation."""
        from . import segment as sg
        sg._require(self, "decode_masks")
        g = self.mask_decoder.g
        if not isinstance(emb, torch.Tensor) or emb.dim() != 4 or tuple(emb.shape[1:]) != (256, g, g):
            raise ValueError(f"decode_masks: emb must be [B, 256, {g}, {g}] (the model's grid), got "
                             f"{tuple(emb.shape) if isinstance(emb, torch.Tensor) else type(emb).__name__}")
        prompts = sg.check_prompts("decode_masks", boxes, points, point_labels, mask_input, emb.shape[0], g, self.mask_decoder)
        logits, iou = sg.select_masks(*self.mask_decoder.decode(emb.to(self.device), *prompts), multimask)
        return sg.Segmentation(logits, iou, (self.cfg.img, self.cfg.img))

    def segment(self, x: torch.Tensor, boxes=None, points=None, point_labels=None, mask_input=None, multimask: bool = False):
        """x [B, 3, S, S] and the prompts of decode_masks, in pixels of x -> vdr.Segmentation: image_encoder followed by
        decode_masks, bit for bit."""
        from . import segment as sg
        sg._require(self, "segment")
        check_batch("segment", x)
        prompts = sg.check_prompts("segment", boxes, points, point_labels, mask_input, x.shape[0], self.mask_decoder.g, self.mask_decoder)   # (before the encoder runs)
        logits, iou = sg.select_masks(*self.mask_decoder.decode(self.image_encoder(x), *prompts), multimask)
        return sg.Segmentation(logits, iou, (self.cfg.img, self.cfg.img))

    def generate_masks(self, x: torch.Tensor, points_per_side: int = 32, points_per_batch: int = 64, pred_iou_thresh: float = 0.88,
                       stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, mask_threshold: float = 0.0,
                       box_nms_thresh: float = 0.7, size=None, min_mask_region_area: int = 0):
        """Segment everything: SAM's automatic mask generator on ONE image x [1, 3, S, S] (or [3, S, S]) -> vdr.MaskSet (vdr/amg.py).
        A points_per_side x points_per_side grid of one-point prompts is decoded points_per_batch at a time into three masks a
        point; every candidate's stability score, area and box at `size` (the input size by default) come from vdr.ops.mask_stats;
        candidates with predicted IoU > pred_iou_thresh and stability > stability_score_thresh (both strict) go through greedy box
        NMS at box_nms_thresh (vdr.ops.nms, best predicted IoU first), and the kept points are decoded once more for their
        logits.  Two host reads in all: the filter flags and the NMS count.  More than 4096 candidates after the filter is a
        ValueError.  min_mask_region_area > 0: segment_anything's small-region removal after the NMS (holes, then islands, below
        that many pixels at `size`, connected components on the device; a second box NMS that prefers unchanged masks; one more
        host read); the MaskSet then carries the cleaned planes.  0 is the path without it: no further launch, the same bits.
        Crop layers and mask-level NMS are out of scope."""
        from . import amg
        return amg.generate(self, x, points_per_side, points_per_batch, pred_iou_thresh, stability_score_thresh, stability_score_offset,
                            mask_threshold, box_nms_thresh, size, min_mask_region_area)

    def propagate_masks(self, x: torch.Tensor, box, index: int, direction: str = "both", margin: float = 8, use_mask_prompt: bool = True,
                        multimask: bool = False, max_batch: int = 16, point_prompt=None):
        """A mask for a whole volume from ONE annotated slice: x [Z, 3, S, S] prepared slices, box (x0, y0, x1, y1) on slice
        `index` in pixels of x -> vdr.VolumeSegmentation.  Slice `index` is decoded from `box`; every further slice gets
        vdr.ops.mask_box of its neighbour's single-mask (token 0) logits, grown by `margin` pixels, as its box and -- with
        use_mask_prompt -- those logits as its mask prompt (False: box-only propagation, the MedSAM way; it needs no
        mask-prompt weights).  An empty mask hands its own box on.  direction: "up" (index + 1 ..), "down" (index - 1 ..) or
        "both": step k then decodes slices index + k and index - k as ONE two-problem call while both exist (a problem's bits
        do not depend on the problem count).  multimask: the stored logits / iou are the highest-IoU of tokens 1..3 instead of
        token 0; the sweep itself always hands token 0 on.  Embeddings come from image_encoder in chunks of max_batch; nothing
        in the sweep synchronises with the host.  point_prompt="inner": every slice after the first also gets ONE positive click,
        vdr.morphology.inner_point of its neighbour's token-0 low-resolution mask (logits > 0, the plane's outside counted as
        clear): the most interior pixel, which keeps a sweep on a thin or concave structure; the label is -1 ("not a point")
        when that mask is empty.  It is computed on the device (vdr_op_distance_transform), needs the point-prompt weights, and
        the sweep still never synchronises.  None (the default) is the sweep without it, bit for bit."""
        from . import morphology as mo
        from . import ops
        from . import segment as sg
        sg._require(self, "propagate_masks")
        if point_prompt not in (None, "inner"):
            raise ValueError(f"propagate_masks: point_prompt must be None or 'inner', got {point_prompt!r}")
        check_batch("propagate_masks", x)
        Z = int(x.shape[0])
        if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < Z:
            raise ValueError(f"propagate_masks: index must be a slice number in [0, {Z}), got {index!r}")
        if direction not in ("both", "up", "down"):
            raise ValueError(f"propagate_masks: direction must be 'both', 'up' or 'down', got {direction!r}")
        if not (isinstance(margin, (int, float)) and margin >= 0):
            raise ValueError(f"propagate_masks: margin must be a number >= 0, got {margin!r}")
        if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
            raise ValueError(f"propagate_masks: max_batch must be a positive integer, got {max_batch!r}")
        b = torch.as_tensor(box)
        if tuple(b.shape) != (4,):
            raise ValueError(f"propagate_masks: box must be (x0, y0, x1, y1), got {tuple(b.shape)}")
        sg.check_boxes("propagate_masks", b.reshape(1, 1, 4))
        dec = self.mask_decoder
        if use_mask_prompt and not dec.has_mask_prompt:
            raise ValueError("propagate_masks: use_mask_prompt needs the checkpoint's prompt_encoder.mask_downscaling.* weights: weights absent "
                             "(use_mask_prompt=False propagates the box alone)")
        if point_prompt is not None and not dec.has_point_prompts:
            raise ValueError("propagate_masks: the checkpoint has no point-prompt weights (point_embeddings.0/1, not_a_point_embed): weights absent")
        g, img, dev = dec.g, self.cfg.img, self.device
        emb = torch.cat([self.image_encoder(x[s0:s0 + max_batch]) for s0 in range(0, Z, max_batch)], dim=0)
        logits = torch.empty((Z, 4 * g, 4 * g), dtype=torch.float32, device=dev)
        iou = torch.empty((Z,), dtype=torch.float32, device=dev)
        boxes = torch.empty((Z, 4), dtype=torch.float32, device=dev)
        area = torch.empty((Z,), dtype=torch.int32, device=dev)

        def step(slices, bx, prev_logits, click=None):
            """decode `slices` from boxes bx [k, 4] (the neighbours' token-0 logits, the neighbours' clicks) -> (their token-0 logits,
            their next boxes, their clicks for the next slice or None)"""
            k = len(slices)
            e = emb[slices[0]:slices[0] + 1] if k == 1 else torch.stack([emb[z] for z in slices])
            lg4, iou4 = dec.decode(e, bx.reshape(k, 1, 4), points=None if click is None else click[0].reshape(k, 1, 1, 2),
                                   labels=None if click is None else click[1].reshape(k, 1, 1),
                                   mask_input=prev_logits.reshape(k, 1, 4 * g, 4 * g) if prev_logits is not None else None)
            lg4, iou4 = lg4[:, 0], iou4[:, 0]                                     # [k, 4, 4g, 4g], [k, 4]
            nxt, ar = ops.mask_box(lg4[:, 0], bx, img, margin=margin, threshold=0.0)
            if multimask:
                j = iou4[:, 1:].argmax(dim=1, keepdim=True)                       # (a device gather: no synchronisation)
                keep = torch.gather(lg4[:, 1:], 1, j[:, :, None, None].expand(-1, 1, 4 * g, 4 * g))[:, 0]
                kiou = torch.gather(iou4[:, 1:], 1, j)[:, 0]
            else:
                keep, kiou = lg4[:, 0], iou4[:, 0]
            for i, z in enumerate(slices):
                logits[z], iou[z], boxes[z], area[z] = keep[i], kiou[i], bx[i], ar[i]
            return lg4[:, 0], nxt, (mo.inner_point(lg4[:, 0] > 0, img, outside=True) if point_prompt else None)

        seed = b.to(dev, torch.float32).reshape(1, 4)
        lg0, nx0, ck0 = step([index], seed, None)
        first = (lg0[0], nx0[0], None if ck0 is None else (ck0[0][0], ck0[1][0]))
        state = {"up": first, "down": first}
        for k in range(1, Z):
            todo = [(d, z) for d, z in (("up", index + k), ("down", index - k)) if direction in ("both", d) and 0 <= z < Z]
            if not todo:
                break
            bx = torch.stack([state[d][1] for d, _ in todo])
            prev = torch.stack([state[d][0] for d, _ in todo]) if use_mask_prompt else None
            click = (torch.stack([state[d][2][0] for d, _ in todo]), torch.stack([state[d][2][1] for d, _ in todo])) if point_prompt else None
            lg, nxt, ck = step([z for _, z in todo], bx, prev, click)
            for i, (d, _) in enumerate(todo):
                state[d] = (lg[i], nxt[i], None if ck is None else (ck[0][i], ck[1][i]))
        return sg.VolumeSegmentation(logits, iou, boxes, area, (img, img))

    # -- input size ------------------------------------------------------------------------------
    def set_input_size(self, height: int, width: int):
        """Run on [B, 3, height, width] images from now on (multiples of the patch side; square or rectangular): the
        learned pos_embed is resampled once on the device (Engine.set_input_size).  ViT / DINOv2 models."""
        check_input_size(self.cfg, height, width)  # (the engine's refusals, for a model that has no engine yet)
        self.engine.set_input_size(height, width)
        return self

    def set_patch_stride(self, stride: int):
        """Run the frozen patch convolution at `stride` (a divisor of the patch side) from now on: every dense output --
        patch_embed, image_encoder, dense_tokens, get_intermediate_layers(reshape=True), get_attention_maps(reshape=True),
        get_dense_descriptor, extract_dense, pipeline.generate_features -- comes on the finer
        ((H - patch) // stride + 1) x ((W - patch) // stride + 1) grid of overlapping patches (Engine.set_patch_stride;
        dino-vit-features' ViTExtractor(stride=...)).  The stride stays in force across input sizes (dynamic_size
        included); stride == patch restores the default.  ViT / DINOv2 / CLIP / SigLIP models."""
        check_patch_stride(self.cfg, stride)  # (as above)
        self.engine.set_patch_stride(stride)
        return self

    @property
    def input_size(self) -> "tuple[int, int]":
        return self.engine.input_size

    @property
    def patch_stride(self) -> int:
        return self.engine.patch_stride

    @property
    def grid(self) -> "tuple[int, int]":
        """(gh, gw) of the dense maps at the input size and patch stride in force."""
        return self.engine.grid

    def _adopt(self, x):
        """dynamic_size: take the size of x as the input size (a no-op when it is the one in force)."""
        if getattr(self, "dynamic_size", False) and x.dim() == 4 and tuple(x.shape[-2:]) != tuple(self.engine.input_size):
            self.set_input_size(int(x.shape[-2]), int(x.shape[-1]))

    def _descriptors(self, x, layer, facet, h, all_rows=False, dtype=torch.bfloat16, saliency=False):
        """The descriptor request of every analysis, for arguments _descriptor_args has passed and a checked [B, 3, H, W]
        batch: the size of x adopted, then ONE forward_descriptors call for the `facet` descriptors of block `layer` (None: the
        last) at hierarchy `h` -> the [B, t, d] buffer.  saliency=True: the same forward also writes the last block's CLS
        attention, mean over the heads; returns (buffer, that attention over the patch columns, min-max normalised per image,
        [B, n] fp32)."""
        i = self.cfg.layers - 1 if layer is None else int(layer)
        self._adopt(x)
        maps = [AttnMap(self.cfg.layers - 1, 1, True)] if saliency else []
        (desc,), _, att = self.engine.forward_descriptors(x, [FacetOut(i, facet, h, bool(all_rows), dtype)], maps=maps)
        return (desc, minmax_normalise(att[0][:, 0, self.cfg.n_prefix:])) if saliency else desc

    def _saliency_ok(self, what):
        if not self.cfg.has_cls:
            raise ValueError(f"{what}: the saliency is the CLS row's attention; the model has no CLS token")

    def _dense_map(self, x, layer=None, facet=None, h=0, dtype=torch.float32, mode=None) -> torch.Tensor:
        """The dense map of x as [B, gh, gw, d], channel-last, from one forward.  facet=None: the model's own dense descriptor
        in fp32 -- the SAM neck output for a windowed model, patch_embed otherwise (mode: another out_mode on the patch grid
        instead, extract_dense's OUT_DENSE); a facet: _descriptors' buffer in `dtype`, viewed on the grid in force."""
        self._adopt(x)
        if facet is not None:
            rows = self._descriptors(x, layer, facet, h, dtype=dtype)
        elif mode is None and self.cfg.window > 0:
            return self.engine.forward(x, L.OUT_ENCODER, torch.float32)  # [B, g, g, C], channel-last already
        else:
            rows = self.engine.forward(x, L.OUT_PATCH_EMBED if mode is None else mode, torch.float32)
        gh, gw = self.engine.grid
        return rows.reshape(rows.shape[0], gh, gw, rows.shape[-1])

    # -- nn.Module-style no-ops so reference code such as model.eval().cuda() keeps working
    def eval(self):
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    # -- R2 -------------------------------------------------------------------------------------
    def patch_embed(self, x: torch.Tensor) -> torch.Tensor:
        """DINOv2 PatchEmbed: [B,3,H,W] -> [B,n,D] (tfds_dense_descriptor.py:128)."""
        self._adopt(x)
        return self.engine.forward(x, L.OUT_PATCH_EMBED, torch.float32)

    def image_encoder(self, x: torch.Tensor) -> torch.Tensor:
        """Channel-first dense map [B,D,h,w], the layout tfds_dense_descriptor.py:123-126 squeezes and
        transposes to (h,w,D).  SAM / MedSAM models return the conv-neck output [B,256,g,g] (g = 64 at 1024^2)."""
        B = x.shape[0]
        if self.cfg.window > 0:
            return self.engine.forward(x, L.OUT_ENCODER, torch.float32).permute(0, 3, 1, 2)
        self._adopt(x)
        gh, gw = self.engine.grid
        dense = self.engine.forward(x, L.OUT_DENSE, torch.float32)
        return dense.reshape(B, gh, gw, self.cfg.dim).permute(0, 3, 1, 2)

    def forward_features(self, x: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
        """[B,3,H,W] -> CLS features [B,D] (the [N,D] matrix embedding_classifier.py consumes)."""
        self._adopt(x)
        return self.engine.forward(x, L.OUT_CLS, out_dtype)

    def dense_tokens(self, x: torch.Tensor, out_dtype=torch.bfloat16) -> torch.Tensor:
        self._adopt(x)
        return self.engine.forward(x, L.OUT_DENSE, out_dtype)

    def _layers_ok(self, what):
        if self.cfg.window > 0:
            raise ValueError(f"{what}: the SAM encoder has no final norm to apply to its blocks' output (and a conv neck); "
                             "intermediate layers are for ViT / DINOv2 models")
        if not self.cfg.layers:
            raise ValueError(f"{what}: the model has no transformer blocks")

    def get_intermediate_layers(self, x: torch.Tensor, n=1, reshape: bool = False, return_class_token: bool = False,
                                norm: bool = True):
        """DINOv2's DinoVisionTransformer.get_intermediate_layers: the residual stream after the chosen blocks (n: the
        last n blocks, or a sequence of block indices), through the final norm when norm=True.  Patch tokens [B, n, D]
        (reshape=True: [B, D, h, w]); with return_class_token a tuple of (patch, cls) pairs, else a tuple of patch
        tensors.  fp32.  All of them come out of one forward (vdr_forward_layers)."""
        self._layers_ok("get_intermediate_layers")
        if return_class_token and not self.cfg.has_cls:
            raise ValueError("get_intermediate_layers: return_class_token needs a model with a CLS token")
        blocks = intermediate_layer_indices(n, self.cfg.layers)
        specs = []
        for i in blocks:
            specs.append(LayerOut(i, L.OUT_DENSE, torch.float32, norm))
            if return_class_token:
                specs.append(LayerOut(i, L.OUT_CLS, torch.float32, norm))
        self._adopt(x)
        got = self.engine.forward_layers(x, specs)
        step = 2 if return_class_token else 1
        patch = got[::step]
        if reshape:
            B, (gh, gw) = patch[0].shape[0], self.engine.grid
            patch = [t.reshape(B, gh, gw, -1).permute(0, 3, 1, 2).contiguous() for t in patch]
        if return_class_token:
            return tuple(zip(patch, got[1::2]))
        return tuple(patch)

    def linear_probe_features(self, x: torch.Tensor, n_last_blocks: int = 4, avgpool: bool = True) -> torch.Tensor:
        """DINOv2's linear-probe descriptor (create_linear_input over get_intermediate_layers(x, n_last_blocks,
        return_class_token=True)): [B, (n_last_blocks + avgpool) * D] fp32, the normalised CLS rows of the last
        n_last_blocks blocks in block order, then (avgpool) the mean of the last block's normalised patch tokens.  One
        forward writes every column slice in place; the patch tokens are never materialised."""
        self._layers_ok("linear_probe_features")
        if not self.cfg.has_cls:
            raise ValueError("linear_probe_features: needs a model with a CLS token")
        blocks = intermediate_layer_indices(int(n_last_blocks), self.cfg.layers)
        B, D = x.shape[0], self.cfg.dim
        out = torch.empty((B, (len(blocks) + int(bool(avgpool))) * D), dtype=torch.float32, device=self.device)
        specs = [LayerOut(i, L.OUT_CLS, out=out[:, k * D:(k + 1) * D]) for k, i in enumerate(blocks)]
        if avgpool:
            specs.append(LayerOut(blocks[-1], L.OUT_POOLED, out=out[:, len(blocks) * D:]))
        self._adopt(x)
        self.engine.forward_layers(x, specs)
        return out

    def _maps_ok(self, what, cls_only):
        if self.cfg.window > 0:
            raise ValueError(f"{what}: attention maps of the SAM encoder (windowed, relative-position attention) are not "
                             "available; they are for ViT / DINOv2 models")
        if not self.cfg.layers:
            raise ValueError(f"{what}: the model has no transformer blocks")
        if cls_only and not self.cfg.has_cls:
            raise ValueError(f"{what}: cls_only needs a model with a CLS token")

    def get_last_selfattention(self, x: torch.Tensor) -> torch.Tensor:
        """DINO's get_last_selfattention: the softmax attention of the last block, every query row, [B, H, N, N] fp32."""
        self._maps_ok("get_last_selfattention", False)
        self._adopt(x)
        N = self.engine.n_tokens
        _, (att,) = self.engine.forward_attn_maps(x, [AttnMap(self.cfg.layers - 1, N)])
        return att

    def get_attention_maps(self, x: torch.Tensor, layers=None, cls_only: bool = True, head_mean: bool = False,
                           reshape: bool = False):
        """Attention maps of the blocks `layers` (block indices; None: the last block), all from one forward, fp32.
        cls_only: the CLS query row only, [B, H, N] ([B, N] with head_mean, the mean over the heads); else the full map
        [B, H, N, N] ([B, N, N]).  reshape (cls_only): the patch key columns only, on the dense-descriptor grid:
        [B, H, g, g] ([B, g, g]).  An int or None gives one tensor, a sequence a tuple in the order given."""
        self._maps_ok("get_attention_maps", cls_only)
        if reshape and not cls_only:
            raise ValueError("get_attention_maps: reshape needs cls_only")
        single = layers is None or isinstance(layers, (int, np.integer))
        idx = block_indices([self.cfg.layers - 1] if layers is None else [layers] if single else layers, self.cfg.layers,
                            "get_attention_maps")
        self._adopt(x)
        N, ncls = self.engine.n_tokens, self.cfg.n_prefix  # (reshape drops the CLS and register key columns)
        _, got = self.engine.forward_attn_maps(x, [AttnMap(i, 1 if cls_only else N, head_mean) for i in idx])
        res = []
        for t in got:
            if cls_only:
                t = t[:, 0] if head_mean else t[:, :, 0]
                if reshape:
                    gh, gw = self.engine.grid
                    t = t[..., ncls:].reshape(*t.shape[:-1], gh, gw)
            res.append(t)
        return res[0] if single else tuple(res)

    def extract_descriptors(self, x: torch.Tensor, layer=None, facet: str = "key", bin: bool = False, include_cls: bool = False,
                            hierarchy: int = 2, reshape: bool = False) -> torch.Tensor:
        """dino-vit-features' ViTExtractor.extract_descriptors: the `facet` ("key" | "query" | "value": block `layer`'s qkv
        linear output, bias included, heads concatenated, before RoPE and before the dh^-0.5 scale; "token": the raw
        residual stream after the block) of block `layer` (None: the last block) as [B, 1, t, d] fp32.  t = the n patch
        rows (include_cls: all N rows, prefix rows first), d = D; bin=True log-bins the patch rows on the grid in force
        (vdr.ops.log_bin at `hierarchy`, 1..3): d = (1 + 8*hierarchy) * D, refused with include_cls as upstream asserts.
        reshape=True (not with include_cls): [B, gh, gw, d] channel-last, as get_dense_descriptor lays its maps out.
        One forward (vdr_forward_facets); a key / query / value request of the last block stops after that block's qkv
        GEMM.  Refusals (ValueError, before any device work): unknown facet, bin with include_cls, hierarchy outside
        1..3, reshape with include_cls, a layer out of range, SAM / token / post-LN / block-less models."""
        h = self._descriptor_args(layer, facet, bin, include_cls, hierarchy)
        if reshape and include_cls:
            raise ValueError("extract_descriptors: reshape needs include_cls=False (the prefix rows have no grid position)")
        if reshape:
            return self._dense_map(x, layer, facet, h, torch.float32)
        return self._descriptors(x, layer, facet, h, include_cls, torch.float32).unsqueeze(1)

    def upsample_descriptors(self, x: torch.Tensor, layer=None, facet="key", bin: bool = False, hierarchy: int = 2, box=None,
                             radius: int = 2, sigma_spatial: float = 1.0, sigma_range: float = 0.1,
                             out_dtype=torch.bfloat16) -> torch.Tensor:
        """Dense descriptors at PIXEL resolution by joint bilateral upsampling guided by x itself (vdr.upsample,
        csrc/upsample.hip): [B, 3, H, W] -> [B, h', w', d] over `box` = (y0, x0, y1, x1) in pixels (None: the whole image), at a
        cost that does not depend on the transformer -- the alternative to a larger input or a finer patch stride.  ONE
        forward_descriptors call for the bf16 `facet` descriptors of block `layer` (extract_descriptors' arguments, bin and
        hierarchy included) and ONE vdr.ops.upsample_guided call on that buffer in place.  facet=None takes the model's own
        dense descriptor in fp32 (the SAM neck output for 'medsam', patch_embed otherwise; rounded once to bf16 by the op).
        sigma_spatial is in grid units (patch strides), sigma_range in units of x.  The input size, patch stride and
        dynamic_size in force apply.  Refusals (ValueError, before any device work): extract_descriptors' own, a layer or bin
        without a facet, and the op's (radius outside 1..3, a box outside the image, non-positive sigmas)."""
        from . import ops
        h = facet_args(self, "upsample_descriptors", layer, facet, bin, hierarchy, "layer and bin need a facet")
        check_batch("upsample_descriptors", x)
        if not 1 <= int(radius) <= ops.UPSAMPLE_MAX_RADIUS:
            raise ValueError(f"upsample_descriptors: radius must be 1..{ops.UPSAMPLE_MAX_RADIUS}, got {radius}")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"upsample_descriptors: out_dtype must be float32 or bfloat16, got {out_dtype}")
        ops.upsample_coefficients(1, sigma_spatial, sigma_range)
        H, W = int(x.shape[-2]), int(x.shape[-1])
        if box is not None:
            y0, x0, y1, x1 = (int(v) for v in box)
            if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
                raise ValueError(f"upsample_descriptors: box {tuple(box)} must be non-empty and inside the {H} x {W} image")
        guide = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
        guide = guide.to(self.device)
        desc = self._dense_map(x, layer, facet, h, torch.bfloat16)
        p, s = int(self.cfg.patch), int(self.engine.patch_stride)  # (a SAM encoder has no other stride than its patch side)
        return ops.upsample_guided(desc, guide, p, s, radius=int(radius), sigma_spatial=sigma_spatial, sigma_range=sigma_range,
                                   box=box, out_dtype=out_dtype)

    def find_correspondences(self, x1: torch.Tensor, x2: torch.Tensor, layer=None, facet: str = "key", bin: bool = True,
                             hierarchy: int = 2, thresh: float = 0.05, keep_descriptors: bool = False, radius=None,
                             keep_cost: bool = False) -> Correspondences:
        """dino-vit-features' point correspondences: mutual cosine nearest neighbours ("best buddies") between the
        descriptors of x1[b] and x2[b], x1 and x2 [B, 3, H, W] of one shape, kept where both patches are salient.
        One forward over cat([x1, x2]) (vdr_forward_facets) writes the bf16 `facet` descriptors of block `layer` (None: the
        last block; upstream uses block 9 of 12), log-binned at `hierarchy` when bin, and the head-mean CLS attention of the
        last block; vdr.ops.nn_cosine then matches the two halves of that one buffer in place -- the t x t similarity
        matrix is never materialised.  The input size, patch stride and dynamic_size in force apply.  Deviations from
        upstream: the saliency averages all heads (upstream: four chosen heads of dino_vits8), and Correspondences.points
        ranks by similarity unless asked for upstream's selection (select="kmeans": k-means over the buddies' descriptors,
        ranked by saliency; it needs keep_descriptors=True, which keeps views of the descriptor buffer in the result).
        radius=r (1..8): both directions are searched inside the (2r + 1) x (2r + 1) window around a patch's own grid position
        instead -- two vdr.ops.local_correlation calls on the same two halves; for adjacent slices and follow-up scans, where
        nothing moves far and a look-alike on the other side of the image is no match.  keep_cost=True (with a radius) keeps
        the 1 -> 2 cost volume in the result.  radius=None is the global match.
        Refusals (ValueError,
        before any device work): extract_descriptors' (unknown facet, hierarchy outside 1..3, a layer out of range, SAM /
        token / post-LN / block-less models), a model without a CLS token, x1 and x2 of different shapes, a radius outside
        1..8, keep_cost without a radius."""
        from . import ops
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        self._saliency_ok("find_correspondences")
        if x1.dim() != 4 or tuple(x1.shape) != tuple(x2.shape):
            raise ValueError(f"find_correspondences: x1 and x2 must be [B, 3, H, W] of the same shape, got {tuple(x1.shape)} "
                             f"and {tuple(x2.shape)}")
        if radius is not None:
            radius = ops.check_local_radius("find_correspondences", radius)
        elif keep_cost:
            raise ValueError("find_correspondences: keep_cost needs a radius (the global match writes no cost volume)")
        B = x1.shape[0]
        desc, sal = self._descriptors(torch.cat([x1.to(self.device), x2.to(self.device)]), layer, facet, h, saliency=True)
        cost12 = None
        if radius is None:
            sim12, nn12, sim21, nn21 = ops.nn_cosine(desc[:B], desc[B:])
        else:
            grid = tuple(self.engine.grid)
            cost12, sim12, nn12 = ops.local_correlation(desc[:B], desc[B:], grid, radius, cost=bool(keep_cost))
            _, sim21, nn21 = ops.local_correlation(desc[B:], desc[:B], grid, radius, cost=False, transposed=True)
        sal1, sal2 = sal[:B], sal[B:]
        mask = ops.best_buddies(nn12, nn21) & (sal1 > thresh) & (torch.gather(sal2, 1, nn12.long()) > thresh)
        res = Correspondences(nn12, sim12, nn21, sim21, sal1, sal2, mask, tuple(self.engine.grid), int(self.engine.patch_stride),
                              int(self.cfg.patch))
        if keep_descriptors:
            res.desc1, res.desc2 = desc[:B], desc[B:]
        res.radius, res.cost12 = radius, cost12
        return res

    def propagate_labels(self, x_src: torch.Tensor, labels_src: torch.Tensor, x_dst: torch.Tensor, n_classes: int, radius: int = 4,
                         k: int = 5, temperature: float = 0.1, layer=None, facet: str = "key", bin: bool = False,
                         hierarchy: int = 2) -> Propagation:
        """DINO's label propagation for one source slice per target slice: every patch of x_dst[b] takes the softmax-weighted
        vote (exp(sim / temperature), normalised) of its k most similar patches of x_src[b] among those at most `radius` grid
        steps from its own position; labels_src [B, gh, gw] integer holds their classes in 0..n_classes-1.  x_src and x_dst are
        [B, 3, H, W] of one shape.  One forward over cat([x_dst, x_src]) writes the bf16 `facet` descriptors (extract_descriptors'
        arguments); one vdr.ops.local_correlation call with the target patches as queries and the source patches as
        candidates writes the [B, t, (2 radius + 1)^2] cost volume -- never a t x t matrix --; vdr.local.topk and
        vdr.knn.vote(weights="softmax") do the rest.  A volume is swept by looping over this, the result's labels becoming
        the next call's labels_src.  No saliency is involved, so the model needs no CLS token.  Several source slices per
        target and soft (probability) labels are propagate_volume's.  The input size, patch stride and dynamic_size in force
        apply.  Refusals (ValueError, before any device work): extract_descriptors' own, shapes of x_src / x_dst / labels_src
        that do not agree with each other or with the grid in force, a radius outside 1..8, k above vdr.local.max_k(grid,
        radius), labels outside 0..n_classes-1, a temperature that is not positive."""
        from . import knn, local, ops
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        check_batch("propagate_labels", x_src)
        if not isinstance(x_dst, torch.Tensor) or tuple(x_src.shape) != tuple(x_dst.shape):
            raise ValueError(f"propagate_labels: x_src and x_dst must be [B, 3, H, W] of the same shape, got {tuple(x_src.shape)} "
                             f"and {tuple(getattr(x_dst, 'shape', ()))}")
        radius = ops.check_local_radius("propagate_labels", radius)
        if int(n_classes) < 1:
            raise ValueError(f"propagate_labels: n_classes must be positive, got {n_classes}")
        if not float(temperature) > 0:
            raise ValueError(f"propagate_labels: temperature must be positive, got {temperature}")
        B, (gh, gw) = x_src.shape[0], self._grid_of("propagate_labels", x_src)
        if not isinstance(labels_src, torch.Tensor) or labels_src.dtype.is_floating_point or labels_src.dtype == torch.bool or \
                tuple(labels_src.shape) != (B, gh, gw):
            raise ValueError(f"propagate_labels: labels_src must be an integer tensor of shape {(B, gh, gw)} (the grid in force), got "
                             f"{getattr(labels_src, 'dtype', type(labels_src).__name__)} {tuple(getattr(labels_src, 'shape', ()))}")
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= local.max_k((gh, gw), radius):
            raise ValueError(f"propagate_labels: k must be 1..{local.max_k((gh, gw), radius)} (the in-grid candidates of a corner patch "
                             f"of a {gh} x {gw} grid at radius {radius}), got {k!r}")
        if labels_src.numel() and (int(labels_src.min()) < 0 or int(labels_src.max()) >= int(n_classes)):
            raise ValueError(f"propagate_labels: labels_src must lie in 0..{int(n_classes) - 1}")
        desc = self._descriptors(torch.cat([x_dst.to(self.device), x_src.to(self.device)]), layer, facet, h)
        cost, _, _ = ops.local_correlation(desc[:B], desc[B:], (gh, gw), radius, best=False)
        idx, val = local.topk(cost, (gh, gw), int(k))
        scores = knn.vote(idx, val, labels_src.to(self.device).reshape(B, gh * gw), int(n_classes), weights="softmax",
                          temperature=float(temperature))
        return Propagation(scores.reshape(B, gh, gw, int(n_classes)), knn.lowest_argmax(scores).reshape(B, gh, gw), idx, val,
                           (int(gh), int(gw)), radius)

    def transfer_labels(self, x_src: torch.Tensor, labels_src: torch.Tensor, x_dst: torch.Tensor, n_classes: int, k: int = 5,
                        temperature: float = 0.1, layer=None, facet: str = "key", bin: bool = False,
                        hierarchy: int = 2) -> Propagation:
        """propagate_labels with the GLOBAL search in place of the window: every patch of x_dst[b] takes the softmax-weighted
        vote of its k most similar patches of x_src[b] wherever they lie -- for slices that are not registered to each
        other (another patient, another orientation), where a window around the own position means nothing.  One forward
        over cat([x_dst, x_src]) writes the bf16 `facet` descriptors; one vdr.ops.knn call with the target patches as queries
        and the source patches as candidates returns the (val, idx) lists -- the t x t similarity matrix is never written --
        and vdr.knn.vote(weights="softmax") votes.  The result is a Propagation with radius None.  Refusals (ValueError,
        before any device work): propagate_labels' own, with k in 1..min(16, t) instead of the window's bound."""
        from . import knn, ops
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        check_batch("transfer_labels", x_src)
        if not isinstance(x_dst, torch.Tensor) or tuple(x_src.shape) != tuple(x_dst.shape):
            raise ValueError(f"transfer_labels: x_src and x_dst must be [B, 3, H, W] of the same shape, got {tuple(x_src.shape)} "
                             f"and {tuple(getattr(x_dst, 'shape', ()))}")
        if int(n_classes) < 1:
            raise ValueError(f"transfer_labels: n_classes must be positive, got {n_classes}")
        if not float(temperature) > 0:
            raise ValueError(f"transfer_labels: temperature must be positive, got {temperature}")
        B, (gh, gw) = x_src.shape[0], self._grid_of("transfer_labels", x_src)
        if not isinstance(labels_src, torch.Tensor) or labels_src.dtype.is_floating_point or labels_src.dtype == torch.bool or \
                tuple(labels_src.shape) != (B, gh, gw):
            raise ValueError(f"transfer_labels: labels_src must be an integer tensor of shape {(B, gh, gw)} (the grid in force), got "
                             f"{getattr(labels_src, 'dtype', type(labels_src).__name__)} {tuple(getattr(labels_src, 'shape', ()))}")
        k = ops.check_knn("transfer_labels", k, "cosine", gh * gw, False)
        if labels_src.numel() and (int(labels_src.min()) < 0 or int(labels_src.max()) >= int(n_classes)):
            raise ValueError(f"transfer_labels: labels_src must lie in 0..{int(n_classes) - 1}")
        desc = self._descriptors(torch.cat([x_dst.to(self.device), x_src.to(self.device)]), layer, facet, h)
        val, idx = ops.knn(desc[:B], desc[B:], k)
        scores = knn.vote(idx, val, labels_src.to(self.device).reshape(B, gh * gw), int(n_classes), weights="softmax",
                          temperature=float(temperature))
        return Propagation(scores.reshape(B, gh, gw, int(n_classes)), knn.lowest_argmax(scores).reshape(B, gh, gw), idx, val,
                           (int(gh), int(gw)), None)

    def fit_knn(self, batches, labels: torch.Tensor, n_classes: int, n_last_blocks: int = 1, avgpool: bool = False, **classifier_kw):
        """The k-NN classifier of this model's frozen features: the bank is linear_probe_features(batch, n_last_blocks, avgpool)
        of every batch of `batches` (an iterable of [B, 3, H, W] tensors, or one such tensor), row after row; labels [N] integer
        classes of those rows.  classifier_kw goes to vdr.knn.KnnClassifier (k, weights, temperature, metric, bank_chunk).
        DINO's evaluation is the defaults: the normalised CLS token of the last block, cosine, softmax votes at T = 0.07."""
        from . import knn
        if isinstance(batches, torch.Tensor):
            batches = [batches]
        feats = [self.linear_probe_features(b.to(self.device), n_last_blocks, avgpool) for b in batches]
        if not feats:
            raise ValueError("fit_knn: no batch was given")
        clf = knn.KnnClassifier(torch.cat(feats), labels, n_classes, **classifier_kw)
        clf.n_last_blocks, clf.avgpool = int(n_last_blocks), bool(avgpool)
        return clf

    def knn_predict(self, x: torch.Tensor, clf):
        """(scores [B, n_classes] fp32, labels [B] int64) of the images x [B, 3, H, W] under a classifier of fit_knn: the same
        features, clf.predict."""
        return clf.predict(self.linear_probe_features(x.to(self.device), clf.n_last_blocks, clf.avgpool))

    def _grid_of(self, what: str, x) -> "tuple[int, int]":
        """The grid the forward of the [B, 3, H, W] batch x will run on, without adopting anything: the grid in force, or with
        dynamic_size the one of x's size; another size is refused (ValueError)."""
        if getattr(self, "dynamic_size", False):
            p, s = int(self.cfg.patch), int(self.engine.patch_stride)
            return (int(x.shape[-2]) - p) // s + 1, (int(x.shape[-1]) - p) // s + 1
        if tuple(x.shape[-2:]) != tuple(self.engine.input_size):
            raise ValueError(f"{what}: the images are {tuple(x.shape[-2:])}, the input size in force {tuple(self.engine.input_size)}")
        gh, gw = self.engine.grid
        return int(gh), int(gw)

    def propagate_volume(self, x: torch.Tensor, labels: torch.Tensor, n_classes: int, index: int = 0, radius: int = 4, k: int = 5,
                         temperature: float = 0.1, n_context: int = 7, direction: str = "both", layer=None, facet: str = "key",
                         bin: bool = False, hierarchy: int = 2, max_batch: int = 16) -> VolumePropagation:
        """DINO's label propagation through a volume: x [Z, 3, H, W] holds the slices in order, `labels` annotates slice
        `index` -- [gh, gw] integer classes in 0..n_classes-1, or [gh, gw, n_classes] float soft scores (finite,
        non-negative) -- and every other slice gets soft scores from the multi-source window vote (vdr.ops.window_vote):
        each patch takes the k most similar source patches at most `radius` grid steps from its own position, over ALL its
        source slices at once, and averages their soft scores with weights exp((sim - best sim) / temperature).
        The sweep runs upwards from index + 1, then downwards from index - 1 with a fresh context (direction: "up" | "down" |
        "both").  The sources of a slice are, IN THIS SLOT ORDER, the annotated slice (slot 0, kept for the whole sweep), then
        the min(n_context, steps so far) most recently propagated slices, nearest first, with the soft scores they received;
        n_context = 0 propagates from the annotated slice alone.  The slot order is part of the result: of two candidates
        with the same similarity the one in the lower slot is taken first.  Slice `index` returns what it was given (hard
        labels as one-hot); a slice the chosen direction does not reach keeps scores 0 and labels -1.
        Device work per slice: one vdr.ops.local_correlation call (pairs = sources, the target expand()ed) and one
        window_vote; no host synchronisation inside the sweep.  The descriptors (extract_descriptors' arguments) come from
        forward_descriptors in chunks of max_batch slices; resident at any time are the annotated slice's map, n_context
        context maps and one chunk, never the volume's.  The input size, patch stride and dynamic_size in force apply.
        Deviations from DINO's eval_video_segmentation: exactly k neighbours (upstream keeps everything tied with the
        k-th), a square window of radius <= 8 patches (upstream: a 12-patch disc), no per-class min-max normalisation of
        the result.  Refusals (ValueError, before any device work): propagate_labels' own, an index outside 0..Z-1,
        n_context outside 0..7, an unknown direction, max_batch < 1, labels whose shape or values do not fit the grid and
        n_classes (1..64), k above 16 or above vdr.local.max_k(grid, radius) -- the candidates of a corner patch in the
        first step, which has one source."""
        from . import knn, local, ops
        what = "propagate_volume"
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        check_batch(what, x)
        radius = ops.check_local_radius(what, radius)
        C = int(n_classes)
        if not 1 <= C <= ops.WINDOW_VOTE_MAX_CLASSES:
            raise ValueError(f"{what}: n_classes must be 1..{ops.WINDOW_VOTE_MAX_CLASSES}, got {n_classes}")
        if not float(temperature) > 0 or float(temperature) == float("inf"):
            raise ValueError(f"{what}: temperature must be positive and finite, got {temperature}")
        Z, (gh, gw) = int(x.shape[0]), self._grid_of(what, x)
        if isinstance(index, bool) or int(index) != index or not 0 <= int(index) < Z:
            raise ValueError(f"{what}: index must be an integer in 0..{Z - 1} (the slices of x), got {index!r}")
        if isinstance(n_context, bool) or int(n_context) != n_context or not 0 <= int(n_context) < ops.WINDOW_VOTE_MAX_SOURCES:
            raise ValueError(f"{what}: n_context must be an integer in 0..{ops.WINDOW_VOTE_MAX_SOURCES - 1}, got {n_context!r}")
        if direction not in ("up", "down", "both"):
            raise ValueError(f"{what}: direction must be 'up', 'down' or 'both', got {direction!r}")
        if isinstance(max_batch, bool) or int(max_batch) != max_batch or int(max_batch) < 1:
            raise ValueError(f"{what}: max_batch must be a positive integer, got {max_batch!r}")
        hard = isinstance(labels, torch.Tensor) and not labels.dtype.is_floating_point and labels.dtype != torch.bool
        if not isinstance(labels, torch.Tensor) or labels.dtype == torch.bool or \
                tuple(labels.shape) != ((gh, gw) if hard else (gh, gw, C)):
            raise ValueError(f"{what}: labels must be an integer tensor of shape {(gh, gw)} or a float tensor of shape {(gh, gw, C)} "
                             f"(the grid in force and n_classes), got {getattr(labels, 'dtype', type(labels).__name__)} "
                             f"{tuple(getattr(labels, 'shape', ()))}")
        k_max = min(local.max_k((gh, gw), radius), ops.WINDOW_VOTE_MAX_K)
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= k_max:
            raise ValueError(f"{what}: k must be 1..{k_max} (at most {ops.WINDOW_VOTE_MAX_K}, and the in-grid candidates of a corner "
                             f"patch of a {gh} x {gw} grid at radius {radius} in the first step), got {k!r}")
        if hard and labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= C):
            raise ValueError(f"{what}: labels must lie in 0..{C - 1}")
        if not hard and not bool((torch.isfinite(labels) & (labels >= 0)).all()):
            raise ValueError(f"{what}: soft labels must be finite and non-negative")
        index, n_context, k, step = int(index), int(n_context), int(k), int(max_batch)

        dev, t = self.device, gh * gw
        given = torch.nn.functional.one_hot(labels.long(), C) if hard else labels
        given = given.to(device=dev, dtype=torch.float32).reshape(t, C)
        scores = torch.zeros((Z, t, C), dtype=torch.float32, device=dev)
        visited = torch.zeros(Z, dtype=torch.bool)
        scores[index], visited[index] = given, True
        anchor = self._descriptors(x[index:index + 1].to(dev), layer, facet, h)[0]
        # the sources in slot order: [0] the annotated slice, [1 ..] the context, nearest first
        bank = torch.empty((1 + n_context,) + tuple(anchor.shape), dtype=anchor.dtype, device=dev)
        soft = torch.empty((1 + n_context, t, C), dtype=torch.float32, device=dev)
        bank[0], soft[0] = anchor, given
        sweeps = ([range(index + 1, Z)] if direction != "down" else []) + ([range(index - 1, -1, -1)] if direction != "up" else [])
        for order in sweeps:
            for c0 in range(0, len(order), step):
                zs = list(order[c0:c0 + step])
                desc = self._descriptors(x[min(zs):max(zs) + 1].to(dev), layer, facet, h)
                for n, z in enumerate(zs, start=c0):  # n: the steps so far in this direction
                    d = desc[z - min(zs)]
                    S = 1 + min(n, n_context)
                    cost, _, _ = ops.local_correlation(d.unsqueeze(0).expand(S, -1, -1), bank[:S], (gh, gw), radius, best=False)
                    got = ops.window_vote(cost.unsqueeze(0), soft[:S].unsqueeze(0), (gh, gw), k, "softmax", float(temperature),
                                          labels=False, neighbours=False)[0][0]
                    scores[z], visited[z] = got, True
                    if n_context:  # the new slice becomes slot 1; the others move up by one and the oldest drops out
                        keep = min(n, n_context - 1)
                        bank[2:2 + keep], soft[2:2 + keep] = bank[1:1 + keep].clone(), soft[1:1 + keep].clone()
                        bank[1], soft[1] = d, got
        lab = torch.where(visited.to(dev).unsqueeze(1), knn.lowest_argmax(scores), -1)
        return VolumePropagation(scores.reshape(Z, gh, gw, C), lab.reshape(Z, gh, gw), (gh, gw), radius, index,
                                 int(self.engine.patch_stride), int(self.cfg.patch))

    def cosegment(self, x: torch.Tensor, k=None, layer=None, facet: str = "key", bin: bool = False, hierarchy: int = 2,
                  thresh: float = 0.065, votes_percentage: float = 75, elbow: float = 0.975, **fit_kwargs) -> Cosegmentation:
        """dino-vit-features' co-segmentation of the B images x [B, 3, H, W]: one forward (vdr_forward_facets) gives the bf16
        `facet` descriptors of block `layer` (None: the last block), log-binned at `hierarchy` when bin, and the head-mean
        CLS attention of the last block, min-max normalised per image as in find_correspondences; the rows are L2-normalised
        in fp32 and rounded once to bf16; ONE joint k-means over all B maps (vdr.kmeans.fit(joint=True); k=None: the elbow
        sweep vdr.kmeans.elbow(ratio=elbow)); then the saliency vote (vdr.kmeans.vote): a cluster is salient when in at least
        votes_percentage % of the images the mean saliency of its patches exceeds thresh.  fit_kwargs go to the fit (init,
        n_init, max_iter, sync_every, seed).  The input size, patch stride and dynamic_size in force apply.
        Deviations from upstream: no GrabCut refinement of the masks, no subsampling of the descriptors before the
        clustering, no part co-segmentation (the second k-means over the foreground); the saliency averages all heads; the
        k-means is this library's Lloyd with a deterministic maximin start (upstream: faiss with random restarts); the elbow
        rule is upstream's as remembered (vdr.kmeans.elbow), not pinned against its code.
        Refusals (ValueError, before any device work): find_correspondences' own, k outside 1..1024 or above B * t."""
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        self._saliency_ok("cosegment")
        check_batch("cosegment", x)
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1024):
            raise ValueError(f"cosegment: k must be None or an integer in 1..1024, got {k!r}")
        from . import kmeans
        self._adopt(x)
        B = x.shape[0]
        gh, gw = self.engine.grid
        if k is not None and int(k) > B * gh * gw:
            raise ValueError(f"cosegment: k = {k} exceeds the {B * gh * gw} patches of the {B} images")
        desc, sal = self._descriptors(x, layer, facet, h, saliency=True)
        rows = torch.nn.functional.normalize(desc.float(), dim=-1, eps=1e-12).to(torch.bfloat16)
        if k is None:
            fit = kmeans.elbow(rows, ratio=float(elbow), joint=True, **fit_kwargs)
        else:
            fit = kmeans.fit(rows, int(k), joint=True, **fit_kwargs)
        labels = fit.labels.reshape(B, gh * gw)
        salient = kmeans.vote(labels, sal, fit.k, float(thresh), float(votes_percentage))
        masks = salient[labels.long()]
        return Cosegmentation(labels.reshape(B, gh, gw), salient, masks.reshape(B, gh, gw), sal.reshape(B, gh, gw), fit)

    def _affinity_graph(self, x, what, layer, facet, bin, hierarchy, tau):
        """one forward for the bf16 `facet` descriptors of x, then their thresholded affinity graph, read in place"""
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        check_batch(what, x)
        if tau != tau:
            raise ValueError(f"{what}: tau is NaN")
        from . import ops
        return ops.affinity_bits(self._descriptors(x, layer, facet, h), tau=tau)

    def tokencut(self, x: torch.Tensor, layer=None, facet: str = "key", bin: bool = False, tau: float = 0.2, eps: float = 1e-5,
                 hierarchy: int = 2, labelling: str = "host"):
        """TokenCut (Wang et al., CVPR 2022) on every image of x [B, 3, H, W]: one forward (vdr_forward_facets) writes the bf16
        `facet` descriptors of block `layer` (None: the last block), log-binned at `hierarchy` when bin;
        vdr.ops.affinity_bits builds the graph cos > tau of each map from that buffer in place, one bit per pair;
        vdr.spectral.tokencut takes the Fiedler vector of (D - W) y = lambda D y, W = eps + (1 - eps) B, splits it at its
        mean and returns the seed's connected component and box (vdr.TokenCut, with the graph in .bits; pixel_box() for pixels).  No mask, no second
        image, no k.  The input size, patch stride and dynamic_size in force apply.  Written from the paper as remembered;
        parity with its code is not pinned.  labelling: "host" (the seed's component by a numpy flood fill per map) or "device" (one
        vdr.ops.connected_components call for all maps; the same masks and boxes).  Refusals (ValueError, before any device work):
        extract_descriptors', a NaN tau, an unknown labelling."""
        from . import spectral
        spectral.check_labelling("tokencut", labelling)
        bits = self._affinity_graph(x, "tokencut", layer, facet, bin, hierarchy, float(tau))
        return spectral.tokencut(bits, tuple(self.engine.grid), eps=float(eps), stride=int(self.engine.patch_stride),
                                 patch=int(self.cfg.patch), **({} if labelling == "host" else {"labelling": labelling}))

    def lost(self, x: torch.Tensor, layer=None, facet: str = "key", k: int = 100, bin: bool = False, hierarchy: int = 2,
             tau: float = 0.0, labelling: str = "host"):
        """LOST (Simeoni et al., BMVC 2021) on every image of x [B, 3, H, W]: the graph cos > 0 of the bf16 `facet` descriptors
        (one forward, vdr.ops.affinity_bits in place), the lowest-degree patch as the seed, the k lowest-degree patches
        adjacent to it as the expansion set, the seed's connected component of that set and its box (vdr.Lost).  tau: the
        threshold of the graph, LOST's 0 by default; descriptors that share a large common component (every cosine positive:
        a complete graph, every degree equal) need a higher one to say anything.  Deviation: LOST compares raw dot products
        with >= 0; here it is cosines > tau.  labelling as tokencut's.  Refusals as
        tokencut's, and k < 1."""
        from . import spectral
        spectral.check_labelling("lost", labelling)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise ValueError(f"lost: k must be a positive integer, got {k!r}")
        bits = self._affinity_graph(x, "lost", layer, facet, bin, hierarchy, float(tau))
        return spectral.lost(bits, tuple(self.engine.grid), k=int(k), stride=int(self.engine.patch_stride), patch=int(self.cfg.patch),
                            **({} if labelling == "host" else {"labelling": labelling}))

    def _anomaly_args(self, what, layer, facet, bin, hierarchy):
        """the device-free refusals shared by fit_anomaly and anomaly_map; returns (hierarchy to ask for, channels)"""
        h = self._descriptor_args(layer, facet, bin, False, hierarchy)
        d = self.cfg.dim * (1 + 8 * h)
        if d % 32:
            raise ValueError(f"{what}: {d} descriptor channels; the Mahalanobis kernel takes multiples of 32")
        return h, d

    def fit_anomaly(self, batches, layer=None, facet: str = "key", bin: bool = False, per_position: bool = False,
                    shrinkage: float = 0.01, ridge: float = 0.0, n_components=None, hierarchy: int = 2):
        """Fit the Gaussian of normal descriptors (vdr.anomaly): `batches` is an iterable of [B, 3, H, W] images of normal
        cases; per batch ONE forward (vdr_forward_facets) for the bf16 `facet` descriptors of block `layer` (None: the last),
        log-binned at `hierarchy` when bin, and ONE vdr.ops.covariance call on that buffer in place; the batches are merged in
        float64 (GaussianAccumulator).  per_position=False: one Gaussian over all patches (Rippel et al.);
        per_position=True: one per patch position (PaDiM), every batch then on the same grid.  shrinkage / ridge /
        n_components: vdr.anomaly.whitening.  Returns a vdr.anomaly.Gaussian that remembers the grid.  The input size, patch
        stride and dynamic_size in force apply.  Refusals (ValueError, before any device work): extract_descriptors' own, a
        descriptor wider than the covariance kernel's 2048 channels; and a per-position batch on another grid than the first."""
        from . import anomaly
        h, d = self._anomaly_args("fit_anomaly", layer, facet, bin, hierarchy)
        if d > 2048:
            raise ValueError(f"fit_anomaly: {d} descriptor channels; the covariance kernel takes at most 2048")
        acc = anomaly.GaussianAccumulator(per_position)
        for x in batches:
            if x.dim() != 4:
                raise ValueError(f"fit_anomaly: every batch must be [B, 3, H, W], got {tuple(x.shape)}")
            self._adopt(x)
            grid = tuple(self.engine.grid)
            if acc.grid is None:
                acc.grid = grid
            elif per_position and grid != acc.grid:
                raise ValueError(f"fit_anomaly: a per-position fit needs one grid; got {grid} after {acc.grid}")
            acc.add(self._descriptors(x, layer, facet, h))
        return acc.finish(shrinkage, ridge, n_components)

    def anomaly_map(self, x: torch.Tensor, gaussian, layer=None, facet: str = "key", bin: bool = False, hierarchy: int = 2):
        """The anomaly map of x [B, 3, H, W] under a fitted vdr.anomaly.Gaussian: ONE forward for the bf16 `facet` descriptors
        (the arguments of the fit) and ONE vdr.ops.mahalanobis call on that buffer in place -> vdr.anomaly.AnomalyMap
        (d2 [B, gh, gw], score [B], upsample()).  The input size, patch stride and dynamic_size in force apply.  Refusals
        (ValueError): extract_descriptors' own, a model of another channel count, a per-position model on another grid."""
        from . import anomaly
        h, d = self._anomaly_args("anomaly_map", layer, facet, bin, hierarchy)
        if not isinstance(gaussian, anomaly.Gaussian):
            raise TypeError("anomaly_map: gaussian must be a vdr.anomaly.Gaussian (fit_anomaly)")
        if int(gaussian.mean.shape[1]) != d:
            raise ValueError(f"anomaly_map: the Gaussian has {int(gaussian.mean.shape[1])} channels, the descriptors {d}")
        check_batch("anomaly_map", x)
        self._adopt(x)
        gh, gw = self.engine.grid
        if gaussian.per_position and (gaussian.grid is not None and tuple(gaussian.grid) != (gh, gw)
                                      or int(gaussian.mean.shape[0]) != gh * gw):
            raise ValueError(f"anomaly_map: the per-position Gaussian was fitted on the grid {gaussian.grid}, the input gives "
                             f"{(gh, gw)}")
        desc = self._descriptors(x, layer, facet, h)
        return anomaly.AnomalyMap(gaussian.score(desc).reshape(desc.shape[0], gh, gw))

    def pca_descriptors(self, x: torch.Tensor, n_components: int = 3, layer=None, facet=None, joint: bool = False,
                        remove_bg: bool = False) -> torch.Tensor:
        """The reference's pca_colorize (visualization_utils.py:49-69) of every image's dense descriptors, on the device:
        [B, 3, H, W] -> [B, gh, gw, n_components] fp32, the leading principal components of each image's map (joint=True:
        of all B maps together, as dino-vit-features' joint PCA), min-max scaled over a problem's whole block;
        remove_bg=True applies the Otsu cut on channel 0 per problem.  One forward, one fit, one projection: facet=None
        takes the model's own dense descriptor (what get_dense_descriptor returns: the SAM neck output for 'medsam',
        patch_embed otherwise), a facet ("key" | "query" | "value" | "token") block `layer`'s bf16 descriptors
        (vdr_forward_facets); vdr.pca.fit and the projection read that buffer in place.  The input size, patch stride and
        dynamic_size in force apply.  Refusals (ValueError, before any device work): extract_descriptors' own;
        n_components outside 1..8; a layer without a facet; a descriptor width that is not a multiple of 32 or exceeds
        2048.  Log-binned descriptors (at ViT-B width bin=True gives (1 + 8 * hierarchy) * 768 > 2048 channels) and the
        library's own top-k solver are keywords of pca_descriptor_maps; this signature stays as it was."""
        return self.pca_descriptor_maps(x, n_components, layer, facet, joint, remove_bg)

    def pca_descriptor_maps(self, x: torch.Tensor, n_components: int = 3, layer=None, facet=None, joint: bool = False,
                            remove_bg: bool = False, bin: bool = False, hierarchy: int = 2, solver: str = "eigh") -> torch.Tensor:
        """pca_descriptors with the log-binning of extract_descriptors and the solver of vdr.pca.fit as keywords (the
        defaults are pca_descriptors, bit for bit).  bin=True (needs a facet): the PCA of the facet's descriptors log-binned
        at `hierarchy` (1..3), (1 + 8 * hierarchy) * D channels.  solver="subspace": the library's top-k solver on the
        smaller side -- a map with fewer rows than channels goes through the t x t Gram matrix, which is what admits more
        than 2048 channels (per image only, at most 4096 patches per image); beyond 2048 channels the colours are the fit's own scores
        (Pca.scores), up to 2048 the projection kernel's as on the covariance side.
        Further refusals (ValueError, before any device work): bin without a facet, an unknown solver, and with
        solver="subspace" a joint PCA of more than 2048 channels, more than 4096 patches per image on the Gram side,
        n_components above rows - 1."""
        from . import pca
        if solver not in pca.SOLVERS:
            raise ValueError(f"pca_descriptors: solver must be one of {pca.SOLVERS}, got {solver!r}")
        h = facet_args(self, "pca_descriptors", layer, facet, bin, hierarchy,
                       f"{'layer' if layer is not None else 'bin'} needs a facet")
        if not 1 <= int(n_components) <= 8:
            raise ValueError(f"pca_descriptors: n_components must be 1..8, got {n_components}")
        d = self.cfg.neck_chans if facet is None and self.cfg.window > 0 else self.cfg.dim
        d *= 1 + 8 * h
        if d % 32 or (d > 2048 and solver == "eigh"):
            raise ValueError(f"pca_descriptors: {d} descriptor channels; the covariance kernel takes multiples of 32 up to 2048 "
                             "(which also excludes log-binned descriptors, bin=True, at ViT-B width)")
        check_batch("pca_descriptors", x)
        if solver == "subspace":  # (fit's refusals, ahead of the forward; a SAM encoder's grid is its configuration's)
            self._adopt(x)
            pca._check_subspace(int(x.shape[0]), self.engine.n_patches, d, int(n_components), joint)
        desc = self._dense_map(x, layer, facet, h, torch.bfloat16)
        B, gh, gw = desc.shape[:3]
        rgb = pca._colorize_maps(desc.reshape(B, gh * gw, desc.shape[-1]), int(n_components), joint, remove_bg, solver)
        return rgb.reshape(B, gh, gw, rgb.shape[-1])

    def _descriptor_args(self, layer, facet, bin, include_cls, hierarchy) -> int:
        """The device-free refusals of a descriptor request; returns the hierarchy to ask for (0 without binning)."""
        check_descriptor_model(self.cfg)
        if bin and not 1 <= int(hierarchy) <= 3:
            raise ValueError(f"hierarchy must be 1, 2 or 3, got {hierarchy}")
        h = int(hierarchy) if bin else 0
        check_facet(facet, h, bool(include_cls))
        if layer is not None and not 0 <= int(layer) < self.cfg.layers:
            raise ValueError(f"layer {layer} out of range 0..{self.cfg.layers - 1}")
        return h

    def get_image_features(self, x: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """The image embedding of a CLIP / SigLIP vision tower, [B, E] fp32 (transformers get_image_features):
        CLIP: visual_projection(post_layernorm(x[:, 0])) -- CLIPVisionModelWithProjection's image_embeds;
        SigLIP: the attention-pooling head over the final-LayerNorm tokens -- SiglipVisionModel's pooler_output.
        normalize=True divides every row by its L2 norm (what the contrastive logits use).  x holds raw [0, 1] values:
        no mean / std normalisation is applied anywhere in this library (include/vdr.h) -- apply the checkpoint's
        image_mean / image_std upstream, as transformers' image processor does."""
        if self.head is None:
            raise ValueError("get_image_features: the model was loaded without a CLIP visual_projection / SigLIP pooling head")
        self._adopt(x)
        f = self.head(self, x)
        return torch.nn.functional.normalize(f, dim=-1) if normalize else f

    def __call__(self, x):
        if self.cfg.window > 0:
            return self.image_encoder(x)
        if isinstance(self.head, _SiglipPoolHead):  # (no CLS token: the pooled feature is SiglipVisionModel's pooler_output)
            return self.get_image_features(x)
        return self.forward_features(x)


def _pad_rows8(w: torch.Tensor) -> torch.Tensor:
    """rows zero-padded to a multiple of 8 (the GEMM's N rule): a weight matrix, or its bias"""
    n = w.shape[0]
    out = torch.zeros(((n + 7) // 8 * 8,) + tuple(w.shape[1:]), dtype=w.dtype)
    out[:n] = w
    return out


class _ClipProjection:
    """CLIPVisionModelWithProjection's visual_projection (nn.Linear, no bias) on the post-LayerNorm CLS rows, through
    vdr_op_linear."""

    def __init__(self, head, dev):
        w = head["head.visual_projection.weight"].float().cpu()
        self.n = w.shape[0]
        self.w = _pad_rows8(w).to(dev, torch.bfloat16).contiguous()

    def __call__(self, model, x):
        from . import ops
        cls = model.engine.forward(x, L.OUT_CLS, torch.bfloat16)
        return ops.linear(cls, self.w, None, epilogue=L.EPI_BIAS)[:, : self.n].float()


class _SiglipPoolHead:
    """transformers SiglipMultiheadAttentionPoolingHead in eval mode: one learned probe attends over every token
    (nn.MultiheadAttention, batch_first), then x + mlp(layernorm(x)) with the tanh-GELU MLP.  The probe's q projection does
    not depend on the image: computed once here in fp32.  Per call: one k/v GEMM over the final-LayerNorm tokens,
    vdr_op_attention_pool, the out-projection, LayerNorm, fc1 with the tanh-GELU epilogue, fc2 with the residual epilogue."""

    def __init__(self, head, cfg, dev):
        W, b = head["head.attention.in_proj_weight"].float().cpu(), head["head.attention.in_proj_bias"].float().cpu()
        D = W.shape[1]
        if D != cfg.dim:
            raise ValueError(f"SigLIP head: in_proj_weight is for width {D}, the model has {cfg.dim}")
        self.D, self.heads, self.head_dim, self.eps = D, cfg.heads, D // cfg.heads, cfg.ln_eps
        self.q = (head["head.probe"].float().cpu().reshape(1, D) @ W[:D].t() + b[:D]).reshape(D).to(dev).contiguous()
        bf = lambda k: head[k].to(dev, torch.bfloat16).contiguous()   # noqa: E731
        f32 = lambda k: head[k].to(dev, torch.float32).contiguous()  # noqa: E731
        self.wkv, self.bkv = W[D:].to(dev, torch.bfloat16).contiguous(), b[D:].to(dev).contiguous()
        self.wo, self.bo = bf("head.attention.out_proj.weight"), f32("head.attention.out_proj.bias")
        self.lnw, self.lnb = f32("head.layernorm.weight"), f32("head.layernorm.bias")
        self.w1, self.b1 = bf("head.mlp.fc1.weight"), f32("head.mlp.fc1.bias")
        self.w2, self.b2 = bf("head.mlp.fc2.weight"), f32("head.mlp.fc2.bias")

    def pooled(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [B, n, D] bf16 (final LayerNorm applied) -> [B, D] fp32"""
        from . import ops
        B, n, D = tokens.shape
        kv = ops.linear(tokens.reshape(B * n, D), self.wkv, self.bkv)                       # [B n, 2D]: k | v
        o = ops.attention_pool(self.q, kv, B, n, self.heads, self.head_dim)                 # [B, D]
        a = ops.linear(o, self.wo, self.bo)
        h = ops.layernorm(a, self.lnw, self.lnb, self.eps)
        u = ops.linear(h, self.w1, self.b1, epilogue=L.EPI_BIAS_GELU_TANH)
        return ops.linear(u, self.w2, self.b2, resid=a, epilogue=L.EPI_BIAS_RESID).float()

    def __call__(self, model, x):
        return self.pooled(model.engine.forward(x, L.OUT_TOKENS, torch.bfloat16))


def load_model(model_name: str, model_path=None, weights=None, device=None, micro_batch: int = 0, streams: int = 0,
               fp8: int = 0, full_last_block: bool = False, ln_fold: bool = True, fp8_cls_bf16: bool = False,
               resid_fp32: bool = False, ln_fin_fused: bool = False, dynamic_size: bool = False, img_size=None,
               stride=None, decoder_eps=None):
    """R1.  model_name: 'dinov2' | 'medsam' (reference names) or any key of ARCHS.
    model_path: a PyTorch state_dict file with the canonical key names; loaded with
    torch.load(weights_only=True).  weights: the same dict passed directly.  A transformers CLIPVisionModel
    [WithProjection] / SiglipVisionModel state_dict (the clip_* / siglip_* entries of ARCHS) is translated on the way in
    (vdr.weights.from_clip_vision_state_dict / from_siglip_vision_state_dict); its projection / pooling head serves
    model.get_image_features(x).  A transformers DINOv3ViTModel / Dinov2Model / Dinov2WithRegistersModel state_dict (the
    dinov3_* / dinov2_*_reg_* entries) is translated too (from_dinov3_vit_state_dict / from_dinov2_hf_state_dict); hub-format
    dinov2_vit*14_reg state_dicts (register_tokens [1, 4, D]) load as they are.  Images are raw [0, 1] here as for every model: no mean / std normalisation is applied.
    fp8=True keeps the qkv / fc1 / fc2 weights as MX-fp8 and runs them on the block-scaled fp8 MFMA
    (BASELINE config 5; pre-LN models).  full_last_block=True: `model(x)` computes every token of the last block
    like the reference does before it keeps x[:, 0] (default: the CLS rows only, same bits).  fp8_cls_bf16=True (fp8 models
    with a CLS token): the MLP of the CLS rows runs on the bf16 weights (vdr_config.fp8_cls_bf16).  resid_fp32=True: the
    residual stream keeps an fp32 master copy (vdr_config.resid_fp32; bf16 path of the plain ViTs).  ln_fin_fused=True:
    the LayerNorm fold's row statistics are finalised inside the residual GEMMs instead of by a launch of their own (A/B).
    dynamic_size=True (ViT / DINOv2 models): the model runs images of any size whose sides are multiples of the patch
    side, resampling pos_embed as DINOv2's interpolate_pos_encoding does (VitDescriptorModel.set_input_size).
    img_size (SAM / MedSAM encoders only; default None = the architecture's own 1024): build the encoder at this square
    input side, as segment_anything's ImageEncoderViT(img_size=...) -- a multiple of the patch side, at most 64 patches a
    side -- and load the checkpoint's native tables into it: pos_embed [1, 64, 64, D] and the global blocks' rel_pos_h / w
    [127, 64] are resampled once on the device (bicubic / get_rel_pos's linear rule).  get_dense_descriptor and
    generate_features then prepare raw slices at that side.
    A SAM / MedSAM checkpoint that also holds prompt_encoder.* / mask_decoder.* (segment_anything's spelling or
    transformers.SamModel's) keeps them: model.has_mask_decoder, model.segment(x, boxes), model.decode_masks(emb, boxes)
    (vdr/segment.py).  decoder_eps: the decoder's three LayerNorm eps (default vdr.segment.SA_EPS, segment_anything's values;
    vdr.segment.HF_EPS is what transformers 5.15 applies).
    stride (default None = the patch side): run the patch convolution at this stride, a divisor of the patch side, for a
    finer dense grid (VitDescriptorModel.set_patch_stride); not for SAM / MedSAM and DINOv3 models."""
    if model_name not in ARCHS:
        raise KeyError(f"unknown model_name {model_name!r}; known: {sorted(ARCHS)} + 'medsam'")
    arch = ARCHS[model_name]
    if img_size is not None:
        if arch.window <= 0:
            raise ValueError(f"img_size is for SAM / MedSAM encoders; '{model_name}' changes size with set_input_size / "
                             "dynamic_size")
        arch = VdrConfig(**{**arch.__dict__, "img": sam_input_side(img_size, arch.patch)})
    cfg = VdrConfig(**{**arch.__dict__, "micro_batch": micro_batch, "streams": streams,
                       "fp8": int(fp8) or int(arch.fp8), "full_last_block": bool(full_last_block),
                       "ln_fold": bool(ln_fold), "fp8_cls_bf16": bool(fp8_cls_bf16), "resid_fp32": bool(resid_fp32),
                       "ln_fin_fused": bool(ln_fin_fused)})
    if weights is None:
        if model_path is None:
            raise ValueError("load_model needs model_path or weights (no network: nothing is downloaded)")
        weights = torch.load(model_path, map_location="cpu", weights_only=True)
    decoder = None
    if arch.window > 0:  # a whole SAM checkpoint: the box-prompt encoder and mask decoder come along (either key spelling)
        from .weights import split_sam_decoder_weights
        weights, decoder = split_sam_decoder_weights(weights)
    if arch.window > 0 and any(k.startswith("vision_encoder.") for k in weights):  # transformers.SamModel's encoder spelling
        from .weights import from_sam_hf_vision_state_dict
        weights = from_sam_hf_vision_state_dict(weights)
    if model_name == "medsam" and any(k.startswith("image_encoder.") for k in weights):
        weights = from_sam_state_dict(weights)
    # transformers CLIPVisionModel[WithProjection] / SiglipVisionModel keys (with or without the vision_model. prefix)
    if any(k.endswith("embeddings.patch_embedding.weight") for k in weights):
        from .weights import from_clip_vision_state_dict, from_siglip_vision_state_dict
        clip = any(k.endswith("embeddings.class_embedding") for k in weights)
        weights = from_clip_vision_state_dict(weights) if clip else from_siglip_vision_state_dict(weights)
    # transformers DINOv3ViTModel keys (embeddings.patch_embeddings.weight, [model.]layer.{i}.*) and Dinov2Model /
    # Dinov2WithRegistersModel keys (embeddings.patch_embeddings.projection.weight, encoder.layer.{i}.*)
    if "embeddings.patch_embeddings.weight" in weights:
        from .weights import from_dinov3_vit_state_dict
        weights = from_dinov3_vit_state_dict(weights)
    elif "embeddings.patch_embeddings.projection.weight" in weights and any(".layer_scale1.lambda1" in k for k in weights):
        from .weights import from_dinov2_hf_state_dict
        weights = from_dinov2_hf_state_dict(weights)
    model = VitDescriptorModel(cfg, weights, model_name, device, dynamic_size=dynamic_size, sized=img_size is not None,
                               decoder_weights=decoder, decoder_eps=decoder_eps)
    model.model_name = model_name
    if stride is not None:
        model.set_patch_stride(stride)
    return model


def get_dense_descriptor(model, img, layer=None, facet=None, bin: bool = False, hierarchy: int = 2) -> np.ndarray:
    """R2: the reference's function (tfds_dense_descriptor.py:110-139), same argument, same result layout.
    img: the RAW slice exactly as the reference passes it -- (h, w) gray or (h, w, 3) colour, values in [0, 1]; it is
    prepared here as `prepare_image` does (tfds_dense_descriptor.py:30-48: gray2rgb + resize to 1024^2 for gray,
    resize to 896^2 for colour, CHW, float32, on the device: vdr.prep.prepare_image) and run through
    `model.image_encoder` ('medsam') or `model.patch_embed` (anything else), returning (h, w, D) float32 numpy.
    Also accepted, for callers that prepared the image themselves: a (3, S, S) or (1, 3, S, S) array / tensor with S
    the model's input side (taken as it is).
    facet ("key" | "query" | "value" | "token"; None: the reference's path above, untouched): the map is
    model.extract_descriptors(t, layer, facet, bin, hierarchy=hierarchy, reshape=True) instead -- (h, w, D), or
    (h, w, (1 + 8*hierarchy)*D) with bin=True."""
    from . import prep
    facet_args(model, "get_dense_descriptor", layer, facet, bin, hierarchy, "layer / bin need a facet")  # (before any device work)
    t = torch.as_tensor(img)
    side = model.cfg.img
    prepared = t.dim() == 4 or (t.dim() == 3 and t.shape[0] == 3 and tuple(t.shape[1:]) == (side, side))
    if prepared:
        t = t.to(torch.float32)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        t = t.to(model.device)
    else:
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
            raise ValueError(f"get_dense_descriptor: a raw (h, w) / (h, w, 3) slice or a prepared (3, {side}, {side}) image, "
                             f"got {tuple(t.shape)}")
        # [1, 3, 1024 | 896, .] float32 on the device; a SAM model loaded with img_size: one resize straight to its side
        t = prep.prepare_image(t, side=side if getattr(model, "sized", False) else None, device=model.device)
        if t.shape[-1] != side:
            raise ValueError(f"prepare_image gives a {t.shape[-1]}^2 image for a {'gray' if torch.as_tensor(img).dim() == 2 else 'colour'} "
                             f"slice, model '{model.model_name}' takes {side}^2 (the reference pairs gray slices with "
                             "'medsam' and colour slices with 'dinov2')")
    if facet is not None:
        return model.extract_descriptors(t, layer, facet, bin, False, hierarchy, reshape=True)[0].cpu().numpy()
    if model.model_name == "medsam":
        f = model.image_encoder(t).cpu().numpy()
        return np.transpose(np.squeeze(f), (1, 2, 0))
    f = model.patch_embed(t).cpu().numpy()
    gh, gw = model.engine.grid
    return f.reshape(gh, gw, f.shape[-1])


def extract_dense(model, images: torch.Tensor, encoder: bool = True, layer=None, facet=None, bin: bool = False,
                  hierarchy: int = 2) -> np.ndarray:
    """Batched counterpart of the reference's per-slice loop (tfds_dense_descriptor.py:271-281):
    [B,3,H,W] -> (B, h, w, D) float32 numpy in one call.  facet (None: that path, untouched): the facet descriptors of
    VitDescriptorModel.extract_descriptors(..., reshape=True) instead, (B, h, w, d)."""
    if facet is not None:
        return model.extract_descriptors(images, layer, facet, bin, False, hierarchy, reshape=True).cpu().numpy()
    facet_args(model, "extract_dense", layer, facet, bin, hierarchy, "layer / bin need a facet")
    return model._dense_map(images, mode=L.OUT_DENSE if encoder else L.OUT_PATCH_EMBED).cpu().numpy()


class _DropIn:
    """nn.Module-style surface the reference's checkpoint helpers use (models_archs.py:14-35: `model.state_dict()`,
    `model.load_state_dict(torch.load(path))`, `model.to(device)`, `model.eval()`)."""

    _sd = None

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def cuda(self, device=None):
        return self

    def state_dict(self):
        self._need_weights()
        return dict(self._sd)

    def _need_weights(self):
        if self._sd is None:
            raise RuntimeError(f"{type(self).__name__}: no weights yet — call load_state_dict(state_dict) first "
                               "(the reference's load(), models_archs.py:32-35)")


class TransformerNoduleClassifier(_DropIn):
    """R3: drop-in for models_archs.TransformerNoduleClassifier in eval mode: the reference's constructor signature
    (models_archs.py:128), then `load_state_dict(sd)` as models_archs.load does (:32-35); `state_dict=` in the
    constructor is a shortcut for the two steps.  model(x[B,S,D]) -> (logits [B,C], cls [B,D])."""

    def __init__(self, input_dim, dim_feedforward, num_heads, num_classes, num_layers, state_dict=None, device=None):
        self.cfg = VdrConfig(img=0, patch=0, in_chans=0, dim=input_dim, heads=num_heads, layers=num_layers,
                             mlp_hidden=dim_feedforward, act="gelu", pre_ln=False, layerscale=False, has_cls=True,
                             has_pos=False, input_ln=True, ln_eps=1e-5)
        self.num_classes, self.num_layers = num_classes, num_layers
        self.engine = Engine(self.cfg, device)
        self.device = self.engine.device
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict, strict=True):
        """state_dict with the reference class's key names (cls_token, norm.*, transformer_encoder.layers.{i}.*,
        classifier.dense1/2.*)."""
        from .weights import from_torch_encoder_state_dict
        sd = {k: v.detach() for k, v in state_dict.items()}
        self.engine.load_weights(from_torch_encoder_state_dict(sd, self.num_layers), strict=strict)
        # MLPLayer head (models_archs.py:186-200): dense1 -> GELU -> dense2, through vdr_op_linear
        self.head = _MlpHead(sd, "classifier", self.device)
        if self.head.n != self.num_classes:
            raise ValueError(f"classifier.dense2 has {self.head.n} rows, model was built for {self.num_classes} classes")
        self._sd = sd
        return self

    def __call__(self, x, lengths=None):
        """x [B,S,D] -> (logits, cls) as the reference.  Variable-length batches (the reference runs batch_size 1
        because its masked-voxel sequences differ in length): pass x padded to the longest sequence plus
        `lengths` [B], or a list of [S_i, D] tensors (padded here)."""
        self._need_weights()
        if isinstance(x, (list, tuple)):
            lengths = [int(t.shape[0]) for t in x]
            x = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(t).float() for t in x], batch_first=True)
        cls = self.engine.forward_tokens(x, L.OUT_CLS, torch.float32, lengths=lengths)
        return self.head(cls), cls


class _MlpHead:
    """models_archs.MLPLayer (:186-200) in eval mode through vdr_op_linear; dense2's rows zero-padded to a multiple
    of 8 (the GEMM's N rule)."""

    def __init__(self, sd, prefix, dev):
        self.w1 = sd[prefix + ".dense1.weight"].to(dev, torch.bfloat16).contiguous()
        self.b1 = sd[prefix + ".dense1.bias"].to(dev, torch.float32).contiguous()
        w2, b2 = sd[prefix + ".dense2.weight"].float().cpu(), sd[prefix + ".dense2.bias"].float().cpu()
        self.n = w2.shape[0]
        self.w2, self.b2 = _pad_rows8(w2).to(dev, torch.bfloat16).contiguous(), _pad_rows8(b2).to(dev)

    def __call__(self, x):
        from . import ops
        hid = ops.linear(x.to(torch.bfloat16).contiguous(), self.w1, self.b1, epilogue=L.EPI_BIAS_GELU)
        out = ops.linear(hid, self.w2, self.b2, epilogue=L.EPI_BIAS)[:, : self.n].float()
        # The device erf-GELU (csrc/vdr_dev.h: max(x, 0) - a 2^Q(a), a = min(|x|, 5.7)) maps a NaN pre-activation to
        # -3e-8 -- v_min / v_max return their non-NaN operand, and a NaN-preserving form costs the VALU-bound fc1 epilogue
        # of the ViTs one to two more instructions per value.  Inside a transformer block the residual stream carries the
        # NaN on; this head has no residual, so a non-finite feature row is handed on here, as torch's gelu would:
        bad = ~torch.isfinite(x.float()).all(dim=-1, keepdim=True)
        return torch.where(bad, torch.full_like(out, float("nan")), out)


class _CrossAttentionCls:
    """CrossAttentionLayer (models_archs.py:174-183 = nn.MultiheadAttention, batch_first, no key padding mask) of
    which the bimodal forward consumes only the CLS query row (`x_attn[:, 0, :]`, :101-102).  Runs on the
    self-attention kernel: keys / values of the other modality are projected into the k | v columns of a packed
    [B*S, 3D] activation whose q columns hold the projected CLS query in row 0 of every sequence; row 0 of the
    kernel's output is then exactly softmax(q_cls K^T / sqrt(dh)) V."""

    def __init__(self, sd, prefix, heads, dev):
        W = sd[prefix + ".multihead_attn.in_proj_weight"].float()
        b = sd[prefix + ".multihead_attn.in_proj_bias"].float()
        D = W.shape[1]
        self.D, self.heads, self.head_dim = D, heads, D // heads  # (nn.MultiheadAttention: heads divides D)
        self.wq, self.bq = W[:D].to(dev, torch.bfloat16).contiguous(), b[:D].to(dev).contiguous()
        self.wkv, self.bkv = W[D:].to(dev, torch.bfloat16).contiguous(), b[D:].to(dev).contiguous()
        self.wo = sd[prefix + ".multihead_attn.out_proj.weight"].to(dev, torch.bfloat16).contiguous()
        self.bo = sd[prefix + ".multihead_attn.out_proj.bias"].to(dev, torch.float32).contiguous()

    def __call__(self, xq, xkv):
        """xq [B, Sq, D], xkv [B, Sk, D] bf16 token sequences -> [B, D] fp32 (row 0 of the attention output)."""
        from . import ops
        B, Sk, D = xkv.shape
        q = ops.linear(xq[:, 0, :].contiguous(), self.wq, self.bq)                      # [B, D]
        qkv = torch.zeros((B, Sk, 3 * D), dtype=torch.bfloat16, device=xkv.device)
        qkv[:, :, D:] = ops.linear(xkv.reshape(B * Sk, D).contiguous(), self.wkv, self.bkv).view(B, Sk, 2 * D)
        qkv[:, 0, :D] = q
        o = ops.attention(qkv.view(B * Sk, 3 * D), B, Sk, self.heads, head_dim=self.head_dim).view(B, Sk, D)[:, 0, :].contiguous()
        return ops.linear(o, self.wo, self.bo).float()


class TransformerNoduleBimodalClassifier(_DropIn):
    """Drop-in for models_archs.TransformerNoduleBimodalClassifier (:38-124) in eval mode: the reference's constructor
    arguments, then `load_state_dict(sd)` (reference key names; `state_dict=` in the constructor is a shortcut);
    `model(x_ct, x_pet)` -> (logits_petct, petct_cls_token, logits_ct, logits_pet); either modality may be None, as in
    the reference."""

    def __init__(self, input_dim, mlp_ratio_ct, mlp_ratio_pet, num_heads_ct, num_heads_pet, num_layers_ct, num_layers_pet,
                 num_classes, state_dict=None, device=None):
        self.engines, self._layers = {}, {}
        for m, ratio, heads, layers in (("ct", mlp_ratio_ct, num_heads_ct, num_layers_ct),
                                        ("pet", mlp_ratio_pet, num_heads_pet, num_layers_pet)):
            cfg = VdrConfig(img=0, patch=0, in_chans=0, dim=input_dim, heads=heads, layers=layers,
                            mlp_hidden=int(ratio * input_dim), act="gelu", pre_ln=False, layerscale=False, has_cls=True,
                            has_pos=False, input_ln=True, ln_eps=1e-5)
            self.engines[m] = Engine(cfg, device)
            self._layers[m] = layers
        self.device = self.engines["ct"].device
        self.num_classes = num_classes
        self._cross_heads = num_heads_ct  # the reference constructs BOTH cross-attention layers with num_heads_ct (:71-72)
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict, strict=True):
        from .weights import from_torch_encoder_state_dict
        sd = {k: v.detach() for k, v in state_dict.items()}
        for m, eng in self.engines.items():
            sub = {"cls_token": sd[f"cls_token_{m}"], "norm.weight": sd[f"norm_{m}.weight"], "norm.bias": sd[f"norm_{m}.bias"]}
            pre = f"transformer_encoder_{m}."
            sub.update({"transformer_encoder." + k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
            eng.load_weights(from_torch_encoder_state_dict(sub, self._layers[m]), strict=strict)
        dev = self.device
        self.cross = {m: _CrossAttentionCls(sd, f"cross_attention_{m}", self._cross_heads, dev) for m in ("ct", "pet")}
        self.heads = {n: _MlpHead(sd, n, dev) for n in ("classifier_ct", "classifier_pet", "projection_petct", "classifier_petct")}
        self._sd = sd
        return self

    def __call__(self, x_ct=None, x_pet=None):
        self._need_weights()
        if x_ct is None and x_pet is None:
            raise AssertionError("At least one modality should be used")  # the reference's assert
        t = {}
        for m, x in (("ct", x_ct), ("pet", x_pet)):
            if x is not None:
                mode = L.OUT_TOKENS if (x_ct is not None and x_pet is not None) else L.OUT_CLS
                t[m] = self.engines[m].forward_tokens(x, mode, torch.bfloat16 if mode == L.OUT_TOKENS else torch.float32)
        if len(t) == 2:
            ct_cls = self.cross["ct"](t["ct"], t["pet"])
            pet_cls = self.cross["pet"](t["pet"], t["ct"])
            logits_ct, logits_pet = self.heads["classifier_ct"](ct_cls), self.heads["classifier_pet"](pet_cls)
            fused = self.heads["projection_petct"](torch.cat([ct_cls, pet_cls], dim=1))
            return self.heads["classifier_petct"](fused), fused, logits_ct, logits_pet
        m = "ct" if "ct" in t else "pet"
        cls = t[m]
        lg = self.heads["classifier_" + m](cls)
        return lg, cls, lg, lg
