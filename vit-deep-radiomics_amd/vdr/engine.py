"""Thin owner of a vdr_handle: weights in, device tensors in/out.  PyTorch supplies device memory,
the current HIP stream and (elsewhere) torch.distributed; all compute is in libvdr.so."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L


@dataclass
class VdrConfig:
    """Mirror of vdr_config (include/vdr.h)."""
    img: int = 224
    patch: int = 16
    in_chans: int = 3
    dim: int = 768
    heads: int = 12
    layers: int = 12
    mlp_hidden: int = 3072
    act: str = "gelu"          # "gelu" (erf) | "swiglu" | "quick_gelu" (CLIP) | "gelu_tanh" (SigLIP)
    pre_ln: bool = True
    layerscale: bool = False
    has_cls: bool = True
    has_pos: bool = True
    input_ln: bool = False
    ln_eps: float = 1e-6
    micro_batch: int = 0
    streams: int = 0
    window: int = 0            # SAM: windowed attention side (14) + decomposed rel-pos
    global_blocks: tuple = ()  # SAM: blocks with global attention (2, 5, 8, 11)
    neck_chans: int = 0        # SAM: conv neck output channels (256)
    fp8: int = 0               # 1: qkv / fc1 / fc2 as MX-fp8 (BASELINE config 5)
    ln_fold: bool = True       # pre-LN image models: LayerNorm folded into the qkv / fc1 GEMMs (False: explicit kernel)
    full_last_block: bool = False  # CLS output: True keeps every row of the last block (default: its CLS rows only,
                               # the same features bit for bit; see vdr_config.full_last_block)
    fp8_cls_bf16: bool = False  # fp8 = 1: the MLP of the CLS rows on the bf16 weights (vdr_config.fp8_cls_bf16)
    resid_fp32: bool = False  # bf16 path: fp32 master copy of the residual stream (vdr_config.resid_fp32)
    ln_fin_fused: bool = False  # LayerNorm fold: the residual GEMMs finalise the row statistics themselves (vdr_config.ln_fin_fused)
    # vdr_config_ext (vdr_create_ext): what came after vdr_config was frozen
    n_register: int = 0        # register tokens between the CLS row and the patch rows (DINOv2-with-registers, DINOv3)
    rope: bool = False         # DINOv3's axial 2-D RoPE on q / k of the patch rows (no pos_embed: has_pos=False)
    rope_theta: float = 100.0

    @property
    def n_patches(self):
        return (self.img // self.patch) ** 2 if self.patch else 0

    @property
    def n_prefix(self):
        """rows in front of the patch rows of an image: the CLS token, then the register tokens"""
        return (1 if self.has_cls else 0) + int(self.n_register)

    @property
    def n_tokens(self):
        return self.n_patches + self.n_prefix

    def to_c(self) -> L.vdr_config:
        c = L.vdr_config()
        c.img, c.patch, c.in_chans, c.dim, c.heads, c.layers = self.img, self.patch, self.in_chans, self.dim, self.heads, self.layers
        c.mlp_hidden = self.mlp_hidden
        c.act = {"swiglu": L.ACT_SWIGLU, "quick_gelu": L.ACT_QUICK_GELU, "gelu_tanh": L.ACT_GELU_TANH}.get(self.act, L.ACT_GELU)
        c.pre_ln, c.layerscale, c.has_cls, c.has_pos = int(self.pre_ln), int(self.layerscale), int(self.has_cls), int(self.has_pos)
        c.input_ln, c.ln_eps, c.micro_batch = int(self.input_ln), float(self.ln_eps), int(self.micro_batch)
        c.streams = int(self.streams)
        c.window, c.neck_chans = int(self.window), int(self.neck_chans)
        c.global_mask = sum(1 << int(i) for i in self.global_blocks)
        c.fp8 = int(self.fp8)
        c.no_ln_fold = int(not self.ln_fold)
        c.full_last_block = int(self.full_last_block)
        c.fp8_cls_bf16 = int(self.fp8_cls_bf16)
        c.resid_fp32 = int(self.resid_fp32)
        c.ln_fin_fused = int(self.ln_fin_fused)
        return c

    def to_c_ext(self) -> L.vdr_config_ext:
        e = L.vdr_config_ext()
        e.size = C.sizeof(L.vdr_config_ext)
        e.n_register, e.rope, e.rope_theta = int(self.n_register), int(bool(self.rope)), float(self.rope_theta)
        return e


_DT = {torch.float32: L.VDR_F32, torch.bfloat16: L.VDR_BF16}


@dataclass
class LayerOut:
    """One output of Engine.forward_layers (vdr_layer_out): the residual stream after block `layer`, through the final
    norm (norm=True) or raw.  out: a caller-owned tensor to write (CLS / POOLED: a [B, D] view whose rows may be
    strided, e.g. a column slice of a wider matrix; DENSE / TOKENS: contiguous), or None to allocate one of `dtype`."""
    layer: int
    mode: int = L.OUT_CLS
    dtype: torch.dtype = torch.float32
    norm: bool = True
    out: "torch.Tensor | None" = None


@dataclass
class AttnMap:
    """One attention map of Engine.forward_attn_maps (vdr_attn_map): softmax(q k^T / sqrt(dh)) of block `layer`, its first
    q_rows query rows (1: the CLS row; N: the full map).  [B, H, q_rows, N], or [B, q_rows, N] with head_mean (the mean
    over the heads).  out: a caller-owned contiguous tensor of that shape, or None to allocate one of `dtype`."""
    layer: int
    q_rows: int = 1
    head_mean: bool = False
    dtype: torch.dtype = torch.float32
    out: "torch.Tensor | None" = None


@dataclass
class FacetOut:
    """One facet descriptor of Engine.forward_descriptors (vdr_facet_out): the "key" / "query" / "value" of block `layer`'s
    attention (the qkv linear's output, before RoPE and scaling) or its "token" (the raw residual stream after the block).
    hierarchy 0: [B, n, D] patch rows, or [B, N, D] with all_rows; hierarchy 1..3: log-binned, [B, n, (1 + 8*hierarchy)*D]
    (patch rows only).  out: a caller-owned contiguous tensor of that shape, or None to allocate one of `dtype`."""
    layer: int
    facet: "str | int" = "key"
    hierarchy: int = 0
    all_rows: bool = False
    dtype: torch.dtype = torch.float32
    out: "torch.Tensor | None" = None


def facet_code(facet) -> int:
    """"token" | "query" | "key" | "value" (or the VDR_FACET_* code) -> the code; ValueError for anything else."""
    if isinstance(facet, str) and facet in L.FACETS:
        return L.FACETS[facet]
    if isinstance(facet, int) and not isinstance(facet, bool) and facet in L.FACETS.values():
        return facet
    raise ValueError(f"facet must be one of {sorted(L.FACETS)}, got {facet!r}")


def check_facet(facet, hierarchy: int, all_rows: bool) -> int:
    """The refusals of a facet request that need no device (ValueError); returns the facet code."""
    code = facet_code(facet)
    if not 0 <= int(hierarchy) <= 3:
        raise ValueError(f"hierarchy must be 1, 2 or 3 (0: no binning), got {hierarchy}")
    if hierarchy and all_rows:
        raise ValueError("a log-binned descriptor takes the patch rows only: bin with include_cls / all_rows is refused")
    return code


def check_descriptor_model(cfg) -> None:
    """Facet descriptors are for pre-LN image models with blocks (vdr_forward_layers' models): ValueError otherwise."""
    if cfg.window > 0:
        raise ValueError("facet descriptors: not for the SAM encoder")
    if not cfg.patch:
        raise ValueError("facet descriptors: image models only (token model)")
    if cfg.layers <= 0:
        raise ValueError("facet descriptors: the model has no blocks")
    if not cfg.pre_ln:
        raise ValueError("facet descriptors: pre-LN models only")


def check_input_size(cfg, height, width) -> "tuple[int, int]":
    """The refusals of set_input_size that need no device (ValueError); returns (height, width) as ints."""
    height, width = int(height), int(width)
    if cfg.window > 0:
        raise ValueError("set_input_size: the SAM encoder's position tables and window partition are tied to its "
                         f"{cfg.img}x{cfg.img} input; its size is chosen at load time (load_model(..., img_size=...))")
    if not cfg.patch:
        raise ValueError("set_input_size: a token model has no input size")
    if height <= 0 or width <= 0 or height % cfg.patch or width % cfg.patch:
        raise ValueError(f"set_input_size: height and width must be positive multiples of patch {cfg.patch}, "
                         f"got {height} x {width}")
    return height, width


def check_patch_stride(cfg, stride) -> int:
    """The refusals of set_patch_stride that need no device (ValueError); returns the stride as an int."""
    stride = int(stride)
    if cfg.window > 0:
        raise ValueError("set_patch_stride: the SAM encoder's position tables and window partition are tied to its grid")
    if not cfg.patch:
        raise ValueError("set_patch_stride: a token model has no patch convolution")
    if cfg.rope:
        raise ValueError("set_patch_stride: not for RoPE models (DINOv3's patch coordinates are defined for "
                         "non-overlapping patches only)")
    if stride <= 0 or stride > cfg.patch or cfg.patch % stride:
        raise ValueError(f"set_patch_stride: stride must be a positive divisor of patch {cfg.patch}, got {stride}")
    return stride


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class Engine:
    def __init__(self, cfg: VdrConfig, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.VdrError(-2, "no HIP device visible: libvdr has no CPU path")
        self.cfg = cfg
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.VdrError(-1, f"libvdr runs on a HIP device, got {dev}")
        # always an indexed device: torch.device("cuda") means the current one
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        h = C.c_void_p()
        cc, ce = cfg.to_c(), cfg.to_c_ext()
        L.check(self.lib.vdr_create_ext(C.byref(cc), C.byref(ce), self.device.index, C.byref(h)))
        self.h = h
        self._ws = None
        self._loaded = False

    def close(self):
        if getattr(self, "h", None):
            self.lib.vdr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -------------------------------------------------------------------------------
    def weight_names(self):
        return [self.lib.vdr_weight_name(self.h, i).decode() for i in range(self.lib.vdr_num_weights(self.h))]

    def load_weights(self, weights: "dict[str, torch.Tensor]", strict=True):
        """weights: canonical (timm/DINOv2-style) names -> tensors in the PyTorch layout."""
        names = self.weight_names()
        missing = [n for n in names if n not in weights]
        if strict and missing:
            raise KeyError(f"missing weights: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for n in names:
            if n not in weights:
                continue
            t = weights[n].detach().to("cpu", torch.float32).contiguous()
            a = t.numpy()
            shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            L.check(self.lib.vdr_set_weight(self.h, n.encode(), a.ctypes.data_as(C.c_void_p), shape, max(a.ndim, 1)), self.h)
        if not missing:
            self.finalize()

    def finalize(self):
        """vdr_finalize: LayerNorm folding, packed GEMM layouts, fp8 copies, rel-pos tables.  Load time (synchronous);
        after it the forward calls neither allocate nor synchronise, so even the first one can be graph-captured."""
        L.check(self.lib.vdr_finalize(self.h), self.h)
        self._loaded = True

    # ---- input size ----------------------------------------------------------------------------
    @property
    def input_size(self) -> "tuple[int, int]":
        """(height, width) the image entry points take: (img, img) until set_input_size."""
        return getattr(self, "_size", None) or (self.cfg.img, self.cfg.img)

    @property
    def patch_stride(self) -> int:
        """Stride of the patch convolution in force: patch until set_patch_stride."""
        return getattr(self, "_stride", None) or self.cfg.patch

    @property
    def grid(self) -> "tuple[int, int]":
        """Patch grid (gh, gw) at the input size and patch stride in force -- ((side - patch) // stride + 1 per side; side //
        patch at the default stride); token i of an image is patch (i // gw, i % gw)."""
        h, w = self.input_size
        p, s = self.cfg.patch, self.patch_stride
        return ((h - p) // s + 1, (w - p) // s + 1) if p else (0, 0)

    @property
    def n_patches(self) -> int:
        gh, gw = self.grid
        return gh * gw

    @property
    def n_tokens(self) -> int:
        return self.n_patches + self.cfg.n_prefix

    def set_input_size(self, height: int, width: int):
        """vdr_set_input_size: run the model on [B, C, height, width] images from now on (sides multiples of patch; square
        or rectangular).  The learned pos_embed is resampled once, on the device, the way DINOv2 / transformers
        interpolate_pos_encoding do (bicubic, align_corners=False; no antialiasing, which upstream's registers variants
        use); (img, img) selects the loaded table again, bit for bit.  A RoPE model (DINOv3) has no table: its cos / sin
        tables are rebuilt for the new grid.
        Load-time class: allocates and synchronises, so call it outside graph capture.  SAM encoders and token models
        are tied to their geometry: ValueError."""
        height, width = check_input_size(self.cfg, height, width)
        L.check(self.lib.vdr_set_input_size(self.h, height, width), self.h)
        self._size = (height, width)

    def set_patch_stride(self, stride: int):
        """vdr_set_patch_stride: run the frozen patch convolution at `stride` <= patch (a divisor of patch) from now on, for
        a ((H - patch) // stride + 1) x ((W - patch) // stride + 1) grid of overlapping patches from the same pixels
        (dino-vit-features' ViTExtractor(stride=...)).  pos_embed's patch rows are resampled to that grid as
        set_input_size resamples them; stride == patch restores the default path, bit for bit.  Load-time class, in any
        order with set_input_size; the stride stays in force across later sizes.  SAM encoders, token models and RoPE
        (DINOv3) models: ValueError."""
        stride = check_patch_stride(self.cfg, stride)
        L.check(self.lib.vdr_set_patch_stride(self.h, stride), self.h)
        self._stride = stride

    def _check_images(self, images: torch.Tensor):
        cfg = self.cfg
        h, w = self.input_size
        if images.dim() != 4 or tuple(images.shape[1:]) != (cfg.in_chans, h, w):
            raise ValueError(f"images must be [B,{cfg.in_chans},{h},{w}], got {tuple(images.shape)}")

    def _adopt_images(self, images: torch.Tensor) -> torch.Tensor:
        """The images of a converting entry point as the library reads them: checked against the size in force, converted to
        float32 unless they are float32 / bfloat16, moved to the engine's device, made contiguous -- a tensor that needs none
        of it is passed on itself, no copy.  forward_into converts nothing and shares the shape check only."""
        self._check_images(images)
        if images.dtype not in _DT:
            images = images.float()
        return images.to(self.device).contiguous()

    # ---- workspace ------------------------------------------------------------------------------
    def _workspace(self, batch: int, seq: int = 0) -> torch.Tensor:
        need = C.c_size_t()
        L.check(self.lib.vdr_workspace_bytes(self.h, batch, seq, C.byref(need)), self.h)
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = None
            # held by the engine: survives torch.cuda.empty_cache() between calls
            # (the reference calls it after every slice, tfds_dense_descriptor.py:137)
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        return self._ws

    def batch_plan(self, batch: int, seq: int = 0) -> "tuple[int, int, int]":
        """vdr_batch_plan: (micro_batch, parts, streams) a forward of `batch` images (sequences of `seq` tokens) runs as --
        the configured micro_batch / streams, or with both 0 the library's default split for this batch."""
        mb, parts, streams = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(self.lib.vdr_batch_plan(self.h, batch, seq, C.byref(mb), C.byref(parts), C.byref(streams)), self.h)
        return mb.value, parts.value, streams.value

    def _run(self, entry, x: torch.Tensor, *args, seq: int = 0):
        """The tail of every forward: entry(handle, x, its dtype, batch, *args, workspace, its size, the current stream),
        checked.  args: what the C entry point takes between `batch` and `workspace`."""
        B = x.shape[0]
        ws = self._workspace(B, seq)
        L.check(entry(self.h, x.data_ptr(), _DT[x.dtype], B, *args, ws.data_ptr(), ws.numel(), _stream_ptr(self.device)), self.h)

    def _out(self, where: str, out, dtype, shape, strided_rows: bool = False) -> torch.Tensor:
        """The output buffer of one struct entry (`where`: "specs[0]", "maps[2]", ...): the caller's `out`, checked -- nothing
        is converted or copied -- or, for None, a fresh one of `dtype`.  strided_rows (shape [B, D]): the rows may lie apart,
        e.g. a column slice of a wider matrix; every other buffer is contiguous."""
        if out is None:
            if dtype not in _DT:
                raise TypeError(f"{where}: dtype must be float32 or bfloat16, got {dtype}")
            out = torch.empty(shape, dtype=dtype, device=self.device)
        if out.dtype not in _DT:
            raise TypeError(f"{where}: out must be float32 or bfloat16, got {out.dtype}")
        if out.device != self.device:
            raise ValueError(f"{where}: out must live on {self.device}")
        if tuple(out.shape) != shape:
            raise ValueError(f"{where}: out must be {shape}, got {tuple(out.shape)}")
        if strided_rows:
            B, D = shape
            if out.stride(1) != 1 or (B > 1 and out.stride(0) < D):
                raise ValueError(f"{where}: out rows must be contiguous and at least D = {D} elements apart")
        elif not out.is_contiguous():
            raise ValueError(f"{where}: out must be contiguous")
        return out

    # ---- hot path --------------------------------------------------------------------------------
    def _out_shape(self, out_mode: int, B: int) -> tuple:
        """what vdr_forward writes for B images (KeyError: no such out_mode)"""
        n, N, D = self.n_patches, self.n_tokens, self.cfg.dim
        gh, gw = self.grid
        return {L.OUT_CLS: (B, D), L.OUT_DENSE: (B, n, D), L.OUT_PATCH_EMBED: (B, n, D), L.OUT_TOKENS: (B, N, D),
                L.OUT_ENCODER: (B, gh, gw, self.cfg.neck_chans)}[out_mode]

    def _forward_into(self, images: torch.Tensor, out: torch.Tensor, out_mode: int) -> torch.Tensor:
        self._run(self.lib.vdr_forward, images, out.data_ptr(), out_mode, _DT[out.dtype])
        return out

    def forward(self, images: torch.Tensor, out_mode: int = L.OUT_CLS, out_dtype=torch.float32) -> torch.Tensor:
        images = self._adopt_images(images)
        out = torch.empty(self._out_shape(out_mode, images.shape[0]), dtype=out_dtype, device=self.device)
        return self._forward_into(images, out, out_mode)

    def forward_into(self, images: torch.Tensor, out: torch.Tensor, out_mode: int = L.OUT_CLS):
        """As forward(), writing into a caller-owned buffer (e.g. this rank's slice of the all-gather buffer).
        Nothing is converted or copied here, so everything is checked: a wrong dtype / layout / size is an error, never
        an out-of-bounds write."""
        self._check_images(images)
        if images.dtype not in _DT or out.dtype not in _DT:
            raise TypeError(f"images / out must be float32 or bfloat16, got {images.dtype} / {out.dtype}")
        if images.device != self.device or out.device != self.device:
            raise ValueError(f"images and out must live on {self.device}")
        if not images.is_contiguous() or not out.is_contiguous():
            raise ValueError("images and out must be contiguous")
        B = images.shape[0]
        per_image = math.prod(self._out_shape(out_mode, 1))
        if out.numel() != B * per_image:  # (the element count, not the shape: callers hand in flat slices of a wider buffer)
            raise ValueError(f"out has {out.numel()} elements, the forward writes {B} x {per_image}")
        return self._forward_into(images, out, out_mode)

    def forward_layers(self, images: torch.Tensor, specs) -> "list[torch.Tensor]":
        """One forward, several outputs from inside the encoder (vdr_forward_layers): specs is a sequence of LayerOut;
        returns their tensors in the same order.  Caller-owned outputs are checked as forward_into checks its buffer,
        nothing is converted or copied."""
        images = self._adopt_images(images)
        specs = list(specs)
        if not specs:
            raise ValueError("forward_layers needs at least one LayerOut")
        arr, outs = self._layer_outs(specs, images.shape[0])
        self._run(self.lib.vdr_forward_layers, images, arr, len(specs))
        return outs

    def forward_attn_maps(self, images: torch.Tensor, maps, outs=()):
        """One forward that writes attention maps (vdr_forward_attn_maps): maps is a sequence of AttnMap, outs an optional
        sequence of LayerOut (forward_layers' outputs, the same bits).  Returns (feature tensors, map tensors), each in
        the order given.  Caller-owned buffers are checked, never converted or copied."""
        images = self._adopt_images(images)
        B = images.shape[0]
        maps, specs = list(maps), list(outs)
        if not maps:
            raise ValueError("forward_attn_maps needs at least one AttnMap")
        arr, feats = self._layer_outs(specs, B)
        marr, got = self._attn_maps(maps, B)
        self._run(self.lib.vdr_forward_attn_maps, images, arr, len(specs), marr, len(maps))
        return feats, got

    def forward_descriptors(self, images: torch.Tensor, facets, outs=(), maps=()):
        """One forward that writes facet descriptors (vdr_forward_facets): facets is a sequence of FacetOut, outs / maps
        optional sequences of LayerOut / AttnMap (forward_layers' and forward_attn_maps' outputs, the same bits).  Returns
        (facet tensors, feature tensors, map tensors), each in the order given.  A last block whose only requests are
        key / query / value facets stops after its qkv GEMM.  Caller-owned buffers are checked, never converted or copied;
        the refusals that need no device (unknown facet, hierarchy outside 0..3, binning with all_rows, SAM / token /
        post-LN / block-less models) are ValueError."""
        facets, specs, maps = list(facets), list(outs), list(maps)
        if not facets:
            raise ValueError("forward_descriptors needs at least one FacetOut")
        for f in facets:
            check_facet(f.facet, f.hierarchy, f.all_rows)
        check_descriptor_model(self.cfg)
        images = self._adopt_images(images)
        B = images.shape[0]
        farr, fgot = self._facet_outs(facets, B)
        arr, feats = self._layer_outs(specs, B)
        marr, mgot = self._attn_maps(maps, B)
        self._run(self.lib.vdr_forward_facets, images, arr, len(specs), marr, len(maps), farr, len(facets))
        return fgot, feats, mgot

    # vdr_layer_out / vdr_attn_map / vdr_facet_out arrays (None: no entry) + their tensors: what shape, which struct fields
    def _layer_outs(self, specs, B):
        if not specs:
            return None, []
        D = self.cfg.dim
        rows = {L.OUT_CLS: None, L.OUT_POOLED: None, L.OUT_DENSE: self.n_patches, L.OUT_TOKENS: self.n_tokens}
        arr, outs = (L.vdr_layer_out * len(specs))(), []
        for k, sp in enumerate(specs):
            if sp.mode not in rows:
                raise ValueError(f"specs[{k}]: mode must be OUT_CLS, OUT_DENSE, OUT_TOKENS or OUT_POOLED, got {sp.mode}")
            r = rows[sp.mode]  # None: [B, D] rows b*ld apart
            out = self._out(f"specs[{k}]", sp.out, sp.dtype, (B, D) if r is None else (B, r, D), strided_rows=r is None)
            ld = 0 if r is not None else out.stride(0) if B > 1 else D
            arr[k].layer, arr[k].out_mode, arr[k].out_dtype = int(sp.layer), int(sp.mode), _DT[out.dtype]
            arr[k].norm, arr[k].ld, arr[k].out = int(bool(sp.norm)), ld, out.data_ptr()
            outs.append(out)
        return arr, outs

    def _attn_maps(self, maps, B):
        if not maps:
            return None, []
        N, H = self.n_tokens, self.cfg.heads
        marr, got = (L.vdr_attn_map * len(maps))(), []
        for k, mp in enumerate(maps):
            q = int(mp.q_rows)
            if not 1 <= q <= N:
                raise ValueError(f"maps[{k}]: q_rows must be in [1, {N}], got {mp.q_rows}")
            out = self._out(f"maps[{k}]", mp.out, mp.dtype, (B, q, N) if mp.head_mean else (B, H, q, N))
            marr[k].layer, marr[k].q_rows, marr[k].head_mean = int(mp.layer), q, int(bool(mp.head_mean))
            marr[k].out_dtype, marr[k].out = _DT[out.dtype], out.data_ptr()
            got.append(out)
        return marr, got

    def _facet_outs(self, facets, B):
        n, N, D = self.n_patches, self.n_tokens, self.cfg.dim
        arr, got = (L.vdr_facet_out * len(facets))(), []
        for k, f in enumerate(facets):
            code = check_facet(f.facet, f.hierarchy, f.all_rows)
            if not 0 <= int(f.layer) < self.cfg.layers:
                raise ValueError(f"facets[{k}]: layer {f.layer} out of range 0..{self.cfg.layers - 1}")
            h = int(f.hierarchy)
            out = self._out(f"facets[{k}]", f.out, f.dtype, (B, n, (1 + 8 * h) * D) if h else (B, N if f.all_rows else n, D))
            arr[k].layer, arr[k].facet, arr[k].hierarchy, arr[k].all_rows = int(f.layer), code, h, int(bool(f.all_rows))
            arr[k].out_dtype, arr[k].out = _DT[out.dtype], out.data_ptr()
            got.append(out)
        return arr, got

    def forward_tokens(self, tokens: torch.Tensor, out_mode: int = L.OUT_CLS, out_dtype=torch.float32,
                       lengths=None) -> torch.Tensor:
        """tokens [B,S,D]; lengths (optional, int [B]): sequence b is tokens[b, :lengths[b]], the rest padding."""
        cfg = self.cfg
        if tokens.dim() != 3 or tokens.shape[2] != cfg.dim:
            raise ValueError(f"tokens must be [B,S,{cfg.dim}], got {tuple(tokens.shape)}")
        if tokens.dtype not in _DT:
            tokens = tokens.float()
        tokens = tokens.to(self.device).contiguous()
        B, S, D = tokens.shape
        c = 1 if cfg.has_cls else 0
        shape = {L.OUT_CLS: (B, D), L.OUT_DENSE: (B, S, D), L.OUT_TOKENS: (B, S + c, D)}[out_mode]
        out = torch.empty(shape, dtype=out_dtype, device=self.device)
        tail = (out.data_ptr(), out_mode, _DT[out_dtype])
        if lengths is None:
            self._run(self.lib.vdr_forward_tokens, tokens, S, *tail, seq=S)
            return out
        lens = torch.as_tensor(lengths, dtype=torch.int32)
        if lens.shape != (B,) or int(lens.min()) < 1 or int(lens.max()) > S:
            raise ValueError(f"lengths must be [B] with 1 <= length <= {S}")
        lens = lens.to(self.device).contiguous()
        self._run(self.lib.vdr_forward_tokens_varlen, tokens, S, lens.data_ptr(), *tail, seq=S)
        return out

    # ---- profiler ---------------------------------------------------------------------------------
    def profile(self, on: bool, classes=None):
        """Bracket kernel launches with HIP events; classes = iterable of class names to restrict to."""
        mask = 0xFFFFFFFF
        if classes is not None:
            names = [self.lib.vdr_kernel_class_name(k).decode() for k in range(L.K_COUNT)]
            mask = 0
            for c in classes:
                mask |= 1 << names.index(c)
        L.check(self.lib.vdr_profile_mask(self.h, mask), self.h)
        L.check(self.lib.vdr_profile_enable(self.h, int(on)), self.h)

    def profile_read(self):
        ms = (C.c_double * L.K_COUNT)()
        ln = (C.c_int64 * L.K_COUNT)()
        fl = (C.c_double * L.K_COUNT)()
        by = (C.c_double * L.K_COUNT)()
        L.check(self.lib.vdr_profile_read(self.h, ms, ln, fl, by, L.K_COUNT), self.h)
        out = {}
        for k in range(L.K_COUNT):
            if ln[k]:
                out[self.lib.vdr_kernel_class_name(k).decode()] = {"ms": ms[k], "launches": int(ln[k]), "flops": fl[k], "bytes": by[k]}
        return out
