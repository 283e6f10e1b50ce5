"""state_dict key translation (host logic, CPU-testable)."""
from __future__ import annotations

import torch


def from_torch_encoder_state_dict(sd, layers: int):
    """nn.TransformerEncoder / TransformerNoduleClassifier keys (models_archs.py:127-139; SURVEY.md §8a
    weight-name map) -> the canonical names vdr_set_weight understands."""
    out = {"cls_token": sd["cls_token"], "input_norm.weight": sd["norm.weight"], "input_norm.bias": sd["norm.bias"]}
    for i in range(layers):
        s, d = f"transformer_encoder.layers.{i}.", f"blocks.{i}."
        out[d + "attn.qkv.weight"] = sd[s + "self_attn.in_proj_weight"]
        out[d + "attn.qkv.bias"] = sd[s + "self_attn.in_proj_bias"]
        out[d + "attn.proj.weight"] = sd[s + "self_attn.out_proj.weight"]
        out[d + "attn.proj.bias"] = sd[s + "self_attn.out_proj.bias"]
        out[d + "mlp.fc1.weight"] = sd[s + "linear1.weight"]
        out[d + "mlp.fc1.bias"] = sd[s + "linear1.bias"]
        out[d + "mlp.fc2.weight"] = sd[s + "linear2.weight"]
        out[d + "mlp.fc2.bias"] = sd[s + "linear2.bias"]
        for n in ("norm1", "norm2"):
            out[d + n + ".weight"] = sd[s + n + ".weight"]
            out[d + n + ".bias"] = sd[s + n + ".bias"]
    return {k: torch.as_tensor(v).detach().to(torch.float32).contiguous() for k, v in out.items()}


def expected_weight_shapes(cfg) -> "dict[str, tuple]":
    """Names and PyTorch shapes a config expects (same list vdr_weight_name enumerates)."""
    D, Fh = cfg.dim, cfg.mlp_hidden
    s = {}
    if cfg.patch:
        s["patch_embed.proj.weight"] = (D, cfg.in_chans, cfg.patch, cfg.patch)
        s["patch_embed.proj.bias"] = (D,)
    if cfg.has_cls:
        s["cls_token"] = (1, 1, D)
    if cfg.has_pos:
        s["pos_embed"] = (1, cfg.n_tokens, D)
    if cfg.input_ln:
        s["input_norm.weight"] = (D,)
        s["input_norm.bias"] = (D,)
    for i in range(cfg.layers):
        p = f"blocks.{i}."
        s[p + "norm1.weight"] = (D,)
        s[p + "norm1.bias"] = (D,)
        s[p + "attn.qkv.weight"] = (3 * D, D)
        s[p + "attn.qkv.bias"] = (3 * D,)
        s[p + "attn.proj.weight"] = (D, D)
        s[p + "attn.proj.bias"] = (D,)
        if cfg.layerscale:
            s[p + "ls1.gamma"] = (D,)
        s[p + "norm2.weight"] = (D,)
        s[p + "norm2.bias"] = (D,)
        if cfg.act == "swiglu":
            s[p + "mlp.w12.weight"] = (2 * Fh, D)
            s[p + "mlp.w12.bias"] = (2 * Fh,)
            s[p + "mlp.w3.weight"] = (D, Fh)
            s[p + "mlp.w3.bias"] = (D,)
        else:
            s[p + "mlp.fc1.weight"] = (Fh, D)
            s[p + "mlp.fc1.bias"] = (Fh,)
            s[p + "mlp.fc2.weight"] = (D, Fh)
            s[p + "mlp.fc2.bias"] = (D,)
        if cfg.layerscale:
            s[p + "ls2.gamma"] = (D,)
    if cfg.pre_ln:
        s["norm.weight"] = (D,)
        s["norm.bias"] = (D,)
    return s


def interpolate_pos_embed(pos_embed, grid, ncls: int = 1, native_grid=None) -> torch.Tensor:
    """Host statement of what vdr_set_input_size builds on the device (DINOv2 / transformers interpolate_pos_encoding):
    pos_embed [1, ncls + g0h*g0w, D] (or [ncls + g0h*g0w, D]) -> fp32 [1, ncls + gh*gw, D]; the first ncls rows copied
    unchanged, the patch rows F.interpolate(size=(gh, gw), mode="bicubic", align_corners=False) evaluated in float64
    and rounded to fp32 once.  grid == the native grid returns the table itself (as fp32).  native_grid: (g0h, g0w),
    default the square grid the row count gives.  Use: the expected table in tests, or resizing a checkpoint's
    pos_embed ahead of time."""
    t = torch.as_tensor(pos_embed).detach().to(torch.float32)
    t = t.reshape(-1, t.shape[-1])
    n0, D = t.shape[0] - ncls, t.shape[1]
    if native_grid is None:
        g0 = int(round(n0 ** 0.5))
        native_grid = (g0, g0)
    g0h, g0w = int(native_grid[0]), int(native_grid[1])
    if g0h * g0w != n0:
        raise ValueError(f"pos_embed has {n0} patch rows, not a {g0h} x {g0w} grid")
    gh, gw = int(grid[0]), int(grid[1])
    if gh <= 0 or gw <= 0:
        raise ValueError(f"grid must be positive, got {gh} x {gw}")
    if (gh, gw) == (g0h, g0w):
        return t.reshape(1, -1, D).clone()
    p = t[ncls:].double().reshape(1, g0h, g0w, D).permute(0, 3, 1, 2)
    p = torch.nn.functional.interpolate(p, size=(gh, gw), mode="bicubic", align_corners=False)
    p = p.permute(0, 2, 3, 1).reshape(gh * gw, D).to(torch.float32)
    return torch.cat([t[:ncls], p], dim=0).reshape(1, -1, D)


def interpolate_rel_pos(table, L: int) -> torch.Tensor:
    """Host statement of what vdr_finalize does to a SAM global block's rel_pos_h / rel_pos_w loaded at another grid
    (vdr_op_interpolate_rel_pos; segment_anything's get_rel_pos): table [L0, D] -> fp32 [L, D],
    F.interpolate(mode="linear", align_corners=False) along the row axis, per channel, evaluated in float64 and rounded
    to fp32 once.  L == L0 returns the table itself (as fp32).  A table for grid side g has L = 2 g - 1 rows."""
    t = torch.as_tensor(table).detach().to(torch.float32)
    if t.dim() != 2:
        raise ValueError(f"rel-pos table must be [L0, D], got {tuple(t.shape)}")
    L = int(L)
    if L <= 0:
        raise ValueError(f"L must be positive, got {L}")
    if L == t.shape[0]:
        return t.clone()
    r = torch.nn.functional.interpolate(t.double().t().unsqueeze(0), size=L, mode="linear", align_corners=False)
    return r[0].t().contiguous().to(torch.float32)


def sam_tables_at(weights, grid: int, global_blocks) -> dict:
    """The weights a SAM encoder with a grid x grid token grid computes with, from a checkpoint learned at another size: pos_embed
    [1, g0, g0, D] and the global blocks' rel-pos tables resampled on the host in float64 (interpolate_pos_embed,
    interpolate_rel_pos) -- what vdr_set_weight + vdr_finalize build on the device.  For tests."""
    g = int(grid)
    out = dict(weights)
    pe = torch.as_tensor(weights["pos_embed"]).float()
    g0 = int(pe.shape[1])
    if g0 != g:
        out["pos_embed"] = interpolate_pos_embed(pe.reshape(1, g0 * g0, -1), (g, g), 0).reshape(1, g, g, -1)
    for i in global_blocks:
        for ax in ("h", "w"):
            k = f"blocks.{i}.attn.rel_pos_{ax}"
            out[k] = interpolate_rel_pos(weights[k], 2 * g - 1)
    return out
