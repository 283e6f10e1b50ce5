"""Guided upsampling of patch-grid maps to pixel resolution: joint bilateral upsampling (Kopf et al. 2007; the parameter-free
filter of FeatUp's JBU up-sampler), guided by the image the descriptors came from.  The filter is ONE op,
vdr.ops.upsample_guided (csrc/upsample.hip); everything here is plain torch on top of it: channel padding for maps that are
not descriptor-shaped (an anomaly map, PCA colours, an eigenvector), label maps through their one-hot encoding, and the
nearest-patch rule restated in integers."""
from __future__ import annotations

import torch

from . import ops


def nearest_patch(size: int, patch: int, stride: int) -> torch.Tensor:
    """[size] int64: the index i0 of the patch nearest to each pixel row (or column) 0 .. size-1 of an image side of `size` =
    patch + (n - 1) * stride pixels -- clamp(floor_div(2Y + 1 - patch + stride, 2 stride), 0, n - 1).  The patch centres lie at
    stride * i + (patch - 1) / 2; equal parity of patch and stride leaves no ties, an even patch under an odd stride sends a
    tie to the upper index."""
    size, p, s = int(size), int(patch), int(stride)
    if p <= 0 or s <= 0 or size < p or (size - p) % s:
        raise ValueError(f"nearest_patch: {size} pixels are no patch + (n - 1) * stride side of patch {patch}, stride {stride}")
    n = (size - p) // s + 1
    Y = torch.arange(size, dtype=torch.int64)
    return torch.div(2 * Y + 1 - p + s, 2 * s, rounding_mode="floor").clamp_(0, n - 1)


def guided(maps: torch.Tensor, guide: torch.Tensor, patch: int, stride: int, radius: int = 2, sigma_spatial: float = 1.0,
           sigma_range: float = 0.1, confidence=None, box=None, out_dtype=None) -> torch.Tensor:
    """Any patch-grid map at pixel resolution: maps [B, gh, gw] or [B, gh, gw, C] (float32 or bfloat16; rounded once to bf16 by
    the op) -> [B, h, w] or [B, h, w, C] over `box` (None: the whole image).  The channels are zero-padded to a multiple of 8
    for the op and sliced off again, so AnomalyMap.d2, PCA colours and the TokenCut eigenvector all go through it.  The other
    arguments are vdr.ops.upsample_guided's."""
    if not isinstance(maps, torch.Tensor) or maps.dim() not in (3, 4) or maps.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("guided: maps must be a [B, gh, gw] or [B, gh, gw, C] float32 or bfloat16 tensor")
    flat = maps.dim() == 3
    x = maps.unsqueeze(-1) if flat else maps
    C = x.shape[-1]
    if C <= 0:
        raise ValueError("guided: maps has no channels")
    pad = -C % 8
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    out = ops.upsample_guided(x, guide, patch, stride, radius=radius, sigma_spatial=sigma_spatial, sigma_range=sigma_range,
                              confidence=confidence, box=box, out_dtype=out_dtype)
    if pad:
        out = out[..., :C]
    return out[..., 0] if flat else out


def guided_labels(labels: torch.Tensor, n: int, guide: torch.Tensor, patch: int, stride: int, radius: int = 2,
                  sigma_spatial: float = 1.0, sigma_range: float = 0.1, confidence=None, box=None) -> torch.Tensor:
    """A label map at pixel resolution: labels [B, gh, gw] integers in 0 .. n-1 -> [B, h, w] int64.  The one-hot encoding is
    upsampled (fp32 out: each channel is the normalised weight its class collects) and the class of the largest channel wins,
    the lowest index on a tie (vdr.knn.lowest_argmax)."""
    from .knn import lowest_argmax
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError("guided_labels: labels must be a [B, gh, gw] integer tensor")
    n = int(n)
    if n < 1:
        raise ValueError(f"guided_labels: n must be >= 1, got {n}")
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= n):
        raise ValueError(f"guided_labels: labels must lie in 0 .. {n - 1}")
    onehot = torch.nn.functional.one_hot(labels.long(), n).to(torch.float32)
    up = guided(onehot, guide, patch, stride, radius=radius, sigma_spatial=sigma_spatial, sigma_range=sigma_range,
                confidence=confidence, box=box, out_dtype=torch.float32)
    return lowest_argmax(up)
