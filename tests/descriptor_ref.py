"""Restatements for the facet descriptors and their log-binning (TEST HELPER): tests/test_descriptors_cpu.py,
tests/test_log_bin_gpu.py, tests/test_descriptors_gpu.py.

Log-bin of F[b, y, x, c] on a gh x gw grid, hierarchy h (include/vdr.h, vdr_op_log_bin): for level k = 0 .. h-1, s = 3^k,
A_k = mean of F over the s x s window centred at (y, x) intersected with the grid (divided by the in-grid count); bins in
the order k, dy in (-s, 0, +s), dx in (-s, 0, +s), (0, 0) skipped for k >= 1; bin j of patch (y, x) is
A_k[clamp(y + dy), clamp(x + dx)]; output [B, gh*gw, (1 + 8h) * C], bin-major.  Two independent fp32 restatements:
  log_bin_brute   from that definition, every window sum exact in float64, then np.float32(sum) / np.float32(count);
  log_bin_pool    the upstream formulation (dino-vit-features' _log_bin): torch.nn.AvgPool2d(3^k, stride=1,
                  padding=3^k // 2, count_include_pad=False) maps plus the clamped gather.

Facets (vdr_forward_facets): q / k / v of block i = F.linear(layer_norm(x_i), Wqkv, bqkv) sliced into thirds -- before
the RoPE rotation of a DINOv3 model -- and token = the raw stream after block i; fp32, or with bf16 rounding emulated at
the device's store points.  The block loop is dinov3_ref.forward's, on the oracle's pieces."""
import numpy as np
import torch

import dinov3_ref as dr
from oracle import vit_oracle as vo


def bin_offsets(hierarchy: int):
    """[(k, dy, dx)] of the 1 + 8h bins, in output order"""
    out = []
    for k in range(hierarchy):
        s = 3 ** k
        for dy in (-s, 0, s):
            for dx in (-s, 0, s):
                if k >= 1 and dy == 0 and dx == 0:
                    continue
                out.append((k, dy, dx))
    return out


def log_bin_brute(x, gh: int, gw: int, hierarchy: int) -> np.ndarray:
    """(a): x [B, gh*gw, C] (array or tensor of fp32-representable values) -> fp32 [B, gh*gw, (1 + 8h) C]"""
    f = np.asarray(torch.as_tensor(x).to(torch.float64).numpy()) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
    B, n, C = f.shape
    assert n == gh * gw
    f = f.reshape(B, gh, gw, C)
    levels = []
    for k in range(hierarchy):
        r = (3 ** k) // 2
        a = np.empty((B, gh, gw, C), dtype=np.float32)
        for y in range(gh):
            y0, y1 = max(y - r, 0), min(y + r, gh - 1)
            for xx in range(gw):
                x0, x1 = max(xx - r, 0), min(xx + r, gw - 1)
                s = f[:, y0:y1 + 1, x0:x1 + 1].sum(axis=(1, 2))  # float64: exact for the inputs the tests use
                cnt = (y1 - y0 + 1) * (x1 - x0 + 1)
                a[:, y, xx] = s.astype(np.float32) / np.float32(cnt)
        levels.append(a)
    offs = bin_offsets(hierarchy)
    out = np.empty((B, gh, gw, len(offs), C), dtype=np.float32)
    for j, (k, dy, dx) in enumerate(offs):
        ys = np.clip(np.arange(gh) + dy, 0, gh - 1)
        xs = np.clip(np.arange(gw) + dx, 0, gw - 1)
        out[:, :, :, j] = levels[k][:, ys][:, :, xs]
    return out.reshape(B, n, len(offs) * C)


def log_bin_pool(x: torch.Tensor, gh: int, gw: int, hierarchy: int) -> torch.Tensor:
    """(b): the upstream formulation on fp32 torch tensors"""
    x = torch.as_tensor(x).to(torch.float32)
    B, n, C = x.shape
    f = x.reshape(B, gh, gw, C).permute(0, 3, 1, 2)  # B, C, gh, gw
    maps = []
    for k in range(hierarchy):
        s = 3 ** k
        maps.append(torch.nn.AvgPool2d(s, stride=1, padding=s // 2, count_include_pad=False)(f))
    ys0, xs0 = torch.arange(gh), torch.arange(gw)
    bins = []
    for k, dy, dx in bin_offsets(hierarchy):
        ys, xs = (ys0 + dy).clamp(0, gh - 1), (xs0 + dx).clamp(0, gw - 1)
        bins.append(maps[k][:, :, ys][:, :, :, xs])
    out = torch.stack(bins, dim=1)  # B, bins, C, gh, gw
    return out.permute(0, 3, 4, 1, 2).reshape(B, n, len(bins) * C).contiguous()


def log_bin_bound(x, hierarchy: int, ref: np.ndarray) -> np.ndarray:
    """Entry-wise bound between two fp32 evaluations of the level means (tests/test_log_bin_gpu.py test 3):
    2 (9^(h-1) - 1) 2^-24 max|x| -- the fp32 summation-order bound of a window of 9^(h-1) terms, once for each side -- plus
    one ulp of the value"""
    amax = float(np.abs(np.asarray(torch.as_tensor(x).float().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)).max())
    return 2.0 * (9 ** (hierarchy - 1) - 1) * 2.0 ** -24 * amax + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def plain(cfg: vo.VitCfg) -> dr.RegCfg:
    """a plain ViT / DINOv2 oracle config as the RegCfg the block loop takes"""
    return dr.RegCfg(cfg, 0, False)


@torch.no_grad()
def facets(rc: dr.RegCfg, w, images, emulate=False):
    """[B, 3, H, W] -> dict of per-block lists: query / key / value [B, N, D] (the qkv linear's output, bias included,
    heads concatenated, BEFORE the rotation of a RoPE model and before any scale) and token [B, N, D] (the raw stream
    after the block).  emulate=True: bf16 rounding where the device stores bf16 (dinov3_ref.forward's points)."""
    from vdr.weights import interpolate_pos_embed
    c, r = rc.vit, vo._r
    eps, P, heads, dh = c.ln_eps, rc.n_prefix, c.heads, c.dim // c.heads
    images = images.to(torch.float32)
    B, _, H, W = images.shape
    grid = (H // c.patch, W // c.patch)
    w = dict(w)
    if c.has_pos and (H, W) != (c.img, c.img):
        w["pos_embed"] = interpolate_pos_embed(w["pos_embed"], grid, 1 if c.has_cls else 0)
    x = r(dr.assemble(rc, w, vo.patch_embed(images, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], c.patch, emulate)), emulate)
    cos, sin = dr.rope_table(grid, dh, rc.rope_theta) if rc.rope else (None, None)
    out = {"query": [], "key": [], "value": [], "token": []}
    for i in range(c.layers):
        p = f"blocks.{i}."
        g1 = w[p + "ls1.gamma"] if c.layerscale else 1.0
        g2 = w[p + "ls2.gamma"] if c.layerscale else 1.0
        h = r(vo.layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"], eps), emulate)
        qkv = r(torch.nn.functional.linear(h, r(w[p + "attn.qkv.weight"], emulate), w[p + "attn.qkv.bias"]), emulate)
        for name, t in zip(("query", "key", "value"), qkv.chunk(3, dim=-1)):
            out[name].append(t.contiguous())
        q, k, v = qkv.reshape(B, -1, 3, heads, dh).permute(2, 0, 3, 1, 4)  # [B, H, N, dh]
        if rc.rope:
            q = torch.cat([q[:, :, :P], r(dr.rotate(q[:, :, P:], cos, sin), emulate)], dim=2)
            k = torch.cat([k[:, :, :P], r(dr.rotate(k[:, :, P:], cos, sin), emulate)], dim=2)
        o = vo.sdpa(q, k, v, emulate).transpose(1, 2).reshape(B, -1, c.dim)
        a = r(o, emulate) @ r(w[p + "attn.proj.weight"], emulate).t() + w[p + "attn.proj.bias"]
        x = r(x + g1 * a, emulate)
        y = r(vo.layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"], eps), emulate)
        x = r(x + g2 * vo.mlp(y, w, p + "mlp.", c.act, emulate), emulate)
        out["token"].append(x)
    return out
