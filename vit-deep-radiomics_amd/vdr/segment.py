"""Box prompt in, mask out: SAM's prompt encoder (boxes only) and mask decoder on the neck output of the library's SAM /
MedSAM encoder (segment_anything's PromptEncoder + MaskDecoder; parity pinned against transformers.SamModel).

A "problem" is one (image, box) pair; P = B * nb, n = g * g cells.  The decode is ONE call of the library's decoder object
(vdr_mask_decode, include/vdr.h): a fixed chain of launches on the caller's stream -- the same number for every B and nb
(MaskDecoder.LAUNCHES) -- of the mask decoder kernels (cross_attention, token_linear, mask_upscale), the GEMM for the
image-side linears and LayerNorm, in a workspace the caller owns.  Per block the three projections that read the image side
(k and v of token-to-image, q of image-to-token) are ONE GEMM on the stacked weight [384, 256]; the positional-encoding terms
pe W^T + b of k and q are fp32 tables of n rows, computed once per decoder in float64 and added inside the attention kernel's
loads.

Out of scope: point and mask prompts, the automatic mask generator, the not_a_point padding path, fp8."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

SA_EPS = dict(ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6)   # segment_anything: nn.LayerNorm's default; LayerNorm2d 1e-6
HF_EPS = dict(ln_eps=1e-6, final_ln_eps=1e-5, ln2d_eps=1e-6)   # transformers.SamModel applies its config's layer_norm_eps


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
        for i in range(self.lib.vdr_mask_decoder_num_weights(h)):
            name = self.lib.vdr_mask_decoder_weight_name(h, i).decode()
            if name not in weights:
                raise ValueError(f"mask decoder: the checkpoint has no {name}")
            t = torch.as_tensor(weights[name]).detach().to(torch.float32).contiguous().cpu()
            shape = (C.c_int64 * t.dim())(*t.shape)
            L.check(self.lib.vdr_mask_decoder_set_weight(h, name.encode(), t.data_ptr(), shape, t.dim()))
        L.check(self.lib.vdr_mask_decoder_finalize(h))

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.vdr_mask_decoder_destroy(h)

    def workspace_bytes(self, problems: int) -> int:
        import ctypes as C
        n = C.c_size_t()
        L.check(self.lib.vdr_mask_decoder_workspace_bytes(self.h, int(problems), C.byref(n)))
        return int(n.value)

    def decode(self, emb: torch.Tensor, boxes: torch.Tensor, workspace=None):
        """emb [B, 256, g, g] on the device (a channel-first view of the encoder's [B, g, g, 256] output is read in place), boxes
        [B, nb, 4] -> (low_res_logits [B, nb, 4, 4g, 4g] fp32, iou [B, nb, 4] fp32) of all four mask tokens: ONE vdr_mask_decode
        call on the current stream.  workspace: a uint8 device tensor of at least workspace_bytes(B * nb), else allocated here."""
        B, nb = int(boxes.shape[0]), int(boxes.shape[1])
        P = B * nb
        emb = emb.to(self.device, torch.float32)
        if emb.permute(0, 2, 3, 1).is_contiguous():
            channels_last = 1
        else:
            emb, channels_last = emb.contiguous(), 0
        bx = boxes.to(self.device, torch.float32).contiguous()
        need = self.workspace_bytes(P)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        logits = torch.empty((B, nb, 4, 4 * self.g, 4 * self.g), dtype=torch.float32, device=self.device)
        iou = torch.empty((B, nb, 4), dtype=torch.float32, device=self.device)
        L.check(self.lib.vdr_mask_decode(self.h, emb.data_ptr(), channels_last, bx.data_ptr(), B, nb, workspace.data_ptr(), workspace.numel(),
                                         logits.data_ptr(), iou.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
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
        raise ValueError(f"{what}: box-prompt segmentation needs a SAM / MedSAM model, got '{getattr(model, 'model_name', type(model).__name__)}'")
    if not getattr(model, "has_mask_decoder", False):
        raise ValueError(f"{what}: the model was loaded without prompt_encoder.* / mask_decoder.* weights (an encoder-only checkpoint)")


def segment_slice(model, img, box, multimask: bool = False, threshold: float = 0.0) -> np.ndarray:
    """get_dense_descriptor's sibling: a RAW (h, w) gray or (h, w, 3) colour slice in [0, 1] and one box (x0, y0, x1, y1) in slice
    pixels -> the (h, w) bool mask at slice resolution ((M, h, w) with multimask).  The slice is prepared as prepare_image
    does, the box scaled by the same factors."""
    from . import prep
    _require(model, "segment_slice")
    t = torch.as_tensor(img)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
        raise ValueError(f"segment_slice: a raw (h, w) / (h, w, 3) slice, got {tuple(t.shape)}")
    b = torch.as_tensor(box)
    if b.shape != (4,):
        raise ValueError(f"segment_slice: box must be (x0, y0, x1, y1), got {tuple(b.shape)}")
    check_boxes("segment_slice", b.reshape(1, 1, 4))
    h, w = int(t.shape[0]), int(t.shape[1])
    side = model.cfg.img
    boxes = torch.tensor([[scale_box(b.tolist(), h, w, side)]], dtype=torch.float64)
    x = prep.prepare_image(t, side=side, device=model.device)
    m = model.segment(x, boxes, multimask=multimask).masks(size=(h, w), threshold=threshold)[0, 0]
    return (m if multimask else m[0]).cpu().numpy()
