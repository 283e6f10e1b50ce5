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


def _hf_vision_tower(sd, what):
    """The shared part of the transformers CLIP / SigLIP vision-tower key translation: sd with or without the
    `vision_model.` prefix -> (canonical tower weights, the stripped dict).  q_proj / k_proj / v_proj are concatenated in
    that order into attn.qkv (rows [q | k | v], the layout of timm's fused qkv), position_embedding.weight [N, D] becomes
    pos_embed [1, N, D], post_layernorm the final norm."""
    sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): torch.as_tensor(v).detach().to(torch.float32)
          for k, v in sd.items() if torch.is_floating_point(torch.as_tensor(v))}
    if "embeddings.patch_embedding.weight" not in sd:
        raise KeyError(f"{what}: no embeddings.patch_embedding.weight -- not a transformers vision-tower state_dict")
    out = {"patch_embed.proj.weight": sd["embeddings.patch_embedding.weight"]}
    D = out["patch_embed.proj.weight"].shape[0]
    out["patch_embed.proj.bias"] = sd.get("embeddings.patch_embedding.bias", torch.zeros(D))  # (CLIP's conv has no bias)
    pos = sd["embeddings.position_embedding.weight"]
    out["pos_embed"] = pos.reshape(1, pos.shape[0], D)
    i = 0
    while f"encoder.layers.{i}.self_attn.q_proj.weight" in sd:
        s, d = f"encoder.layers.{i}.", f"blocks.{i}."
        for t in ("weight", "bias"):
            out[d + "attn.qkv." + t] = torch.cat([sd[s + f"self_attn.{p}_proj.{t}"] for p in ("q", "k", "v")], dim=0)
            out[d + "attn.proj." + t] = sd[s + "self_attn.out_proj." + t]
            out[d + "norm1." + t] = sd[s + "layer_norm1." + t]
            out[d + "norm2." + t] = sd[s + "layer_norm2." + t]
            out[d + "mlp.fc1." + t] = sd[s + "mlp.fc1." + t]
            out[d + "mlp.fc2." + t] = sd[s + "mlp.fc2." + t]
        i += 1
    for t in ("weight", "bias"):
        out["norm." + t] = sd["post_layernorm." + t]
    return out, sd


def from_clip_vision_state_dict(sd):
    """transformers CLIPVisionModel / CLIPVisionModelWithProjection state_dict (OpenAI CLIP and its descendants:
    PubMedCLIP, QuiltNet, PLIP) -> the canonical names vdr_set_weight understands: class_embedding [D] -> cls_token
    [1, 1, D], pre_layrnorm -> input_norm, the bias-free patch conv gets a zero bias.  visual_projection.weight [E, D]
    (when the checkpoint has it) is returned as head.visual_projection.weight: it is not a weight of the encoder."""
    out, sd = _hf_vision_tower(sd, "from_clip_vision_state_dict")
    out["cls_token"] = sd["embeddings.class_embedding"].reshape(1, 1, -1)
    for t in ("weight", "bias"):
        out["input_norm." + t] = sd["pre_layrnorm." + t]
    if "visual_projection.weight" in sd:
        out["head.visual_projection.weight"] = sd["visual_projection.weight"]
    return {k: v.contiguous() for k, v in out.items()}


def from_siglip_vision_state_dict(sd):
    """transformers SiglipVisionModel state_dict -> the canonical names (no CLS token, no input norm).  The attention-
    pooling head (head.probe, head.attention.in_proj_weight / in_proj_bias / out_proj.*, head.layernorm.*, head.mlp.fc1 /
    fc2.*) keeps its names under head.*: it is not a weight of the encoder."""
    out, sd = _hf_vision_tower(sd, "from_siglip_vision_state_dict")
    out.update({k: v for k, v in sd.items() if k.startswith("head.")})
    return {k: v.contiguous() for k, v in out.items()}


def _f32(sd):
    return {k: torch.as_tensor(v).detach().to(torch.float32) for k, v in sd.items() if torch.is_floating_point(torch.as_tensor(v))}


def from_dinov3_vit_state_dict(sd):
    """transformers DINOv3ViTModel state_dict (layers under `model.layer.{i}.` or `layer.{i}.`) -> the canonical names:
    q_proj / k_proj / v_proj concatenated into attn.qkv (k_proj has no bias: a zero k bias is supplied), o_proj ->
    attn.proj, layer_scale{1,2}.lambda1 -> ls{1,2}.gamma, up_proj / down_proj -> mlp.fc1 / fc2 or, gated,
    cat(gate_proj, up_proj) -> mlp.w12 and down_proj -> mlp.w3 (silu(gate) * up: the SwiGLU epilogue).  mask_token is
    dropped.  There is no pos_embed: the model is built with has_pos=False, rope=True.  (The key names of the original
    facebookresearch/dinov3 checkpoints are not handled.)"""
    sd = _f32(sd)
    if "embeddings.patch_embeddings.weight" not in sd:
        raise KeyError("from_dinov3_vit_state_dict: no embeddings.patch_embeddings.weight -- not a transformers DINOv3ViTModel state_dict")
    pre = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    out = {"patch_embed.proj.weight": sd["embeddings.patch_embeddings.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.bias"],
           "cls_token": sd["embeddings.cls_token"].reshape(1, 1, -1)}
    D = out["patch_embed.proj.weight"].shape[0]
    if "embeddings.register_tokens" in sd and sd["embeddings.register_tokens"].numel():
        out["register_tokens"] = sd["embeddings.register_tokens"].reshape(1, -1, D)
    i = 0
    while f"{pre}{i}.attention.q_proj.weight" in sd:
        s, d = f"{pre}{i}.", f"blocks.{i}."
        att = s + "attention."
        out[d + "attn.qkv.weight"] = torch.cat([sd[att + f"{p}_proj.weight"] for p in ("q", "k", "v")], dim=0)
        out[d + "attn.qkv.bias"] = torch.cat([sd.get(att + f"{p}_proj.bias", torch.zeros(D)) for p in ("q", "k", "v")], dim=0)
        out[d + "attn.proj.weight"] = sd[att + "o_proj.weight"]
        out[d + "attn.proj.bias"] = sd.get(att + "o_proj.bias", torch.zeros(D))
        out[d + "ls1.gamma"], out[d + "ls2.gamma"] = sd[s + "layer_scale1.lambda1"], sd[s + "layer_scale2.lambda1"]
        for n in ("norm1", "norm2"):
            for t in ("weight", "bias"):
                out[d + f"{n}.{t}"] = sd[s + f"{n}.{t}"]
        Fh = sd[s + "mlp.up_proj.weight"].shape[0]
        bias = lambda k, n: sd.get(s + f"mlp.{k}.bias", torch.zeros(n))  # noqa: E731
        if s + "mlp.gate_proj.weight" in sd:
            out[d + "mlp.w12.weight"] = torch.cat([sd[s + "mlp.gate_proj.weight"], sd[s + "mlp.up_proj.weight"]], dim=0)
            out[d + "mlp.w12.bias"] = torch.cat([bias("gate_proj", Fh), bias("up_proj", Fh)], dim=0)
            out[d + "mlp.w3.weight"], out[d + "mlp.w3.bias"] = sd[s + "mlp.down_proj.weight"], bias("down_proj", D)
        else:
            out[d + "mlp.fc1.weight"], out[d + "mlp.fc1.bias"] = sd[s + "mlp.up_proj.weight"], bias("up_proj", Fh)
            out[d + "mlp.fc2.weight"], out[d + "mlp.fc2.bias"] = sd[s + "mlp.down_proj.weight"], bias("down_proj", D)
        i += 1
    out["norm.weight"], out["norm.bias"] = sd["norm.weight"], sd["norm.bias"]
    return {k: v.contiguous() for k, v in out.items()}


def from_dinov2_hf_state_dict(sd):
    """transformers Dinov2Model / Dinov2WithRegistersModel state_dict -> the canonical (hub DINOv2) names: query / key /
    value concatenated into attn.qkv, attention.output.dense -> attn.proj, layer_scale{1,2}.lambda1 -> ls{1,2}.gamma,
    mlp.fc1 / fc2 or (SwiGLU) mlp.weights_in / weights_out -> mlp.w12 / w3, layernorm -> norm, position_embeddings ->
    pos_embed [1, 1 + n, D], register_tokens kept [1, R, D] when the model has them.  mask_token is dropped."""
    sd = _f32(sd)
    if "embeddings.patch_embeddings.projection.weight" not in sd:
        raise KeyError("from_dinov2_hf_state_dict: no embeddings.patch_embeddings.projection.weight -- not a transformers "
                       "Dinov2Model / Dinov2WithRegistersModel state_dict")
    out = {"patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"],
           "cls_token": sd["embeddings.cls_token"].reshape(1, 1, -1),
           "pos_embed": sd["embeddings.position_embeddings"]}
    D = out["patch_embed.proj.weight"].shape[0]
    if "embeddings.register_tokens" in sd and sd["embeddings.register_tokens"].numel():
        out["register_tokens"] = sd["embeddings.register_tokens"].reshape(1, -1, D)
    i = 0
    while f"encoder.layer.{i}.attention.attention.query.weight" in sd:
        s, d = f"encoder.layer.{i}.", f"blocks.{i}."
        for t in ("weight", "bias"):
            out[d + "attn.qkv." + t] = torch.cat([sd[s + f"attention.attention.{p}.{t}"] for p in ("query", "key", "value")], dim=0)
            out[d + "attn.proj." + t] = sd[s + "attention.output.dense." + t]
            out[d + "norm1." + t], out[d + "norm2." + t] = sd[s + "norm1." + t], sd[s + "norm2." + t]
            if s + "mlp.weights_in.weight" in sd:
                out[d + "mlp.w12." + t], out[d + "mlp.w3." + t] = sd[s + "mlp.weights_in." + t], sd[s + "mlp.weights_out." + t]
            else:
                out[d + "mlp.fc1." + t], out[d + "mlp.fc2." + t] = sd[s + "mlp.fc1." + t], sd[s + "mlp.fc2." + t]
        out[d + "ls1.gamma"], out[d + "ls2.gamma"] = sd[s + "layer_scale1.lambda1"], sd[s + "layer_scale2.lambda1"]
        i += 1
    out["norm.weight"], out["norm.bias"] = sd["layernorm.weight"], sd["layernorm.bias"]
    return {k: v.contiguous() for k, v in out.items()}


def rope2d_table(grid, head_dim: int, theta: float = 100.0):
    """Host statement of vdr_op_rope2d_table (DINOv3's axial 2-D RoPE): (cos, sin), fp32 [gh*gw, head_dim/2] each -- angle,
    cos and sin evaluated in float64 and rounded once.  Patch (y, x): cy = 2 (y + 0.5) / gh - 1, cx = 2 (x + 0.5) / gw - 1,
    inv_freq[i] = theta^(-4 i / head_dim); angles [2 pi cy inv_freq | 2 pi cx inv_freq]."""
    import math
    gh, gw, q = int(grid[0]), int(grid[1]), int(head_dim) // 4
    inv = float(theta) ** (-torch.arange(q, dtype=torch.float64) / q)
    cy = 2.0 * (torch.arange(gh, dtype=torch.float64) + 0.5) / gh - 1.0
    cx = 2.0 * (torch.arange(gw, dtype=torch.float64) + 0.5) / gw - 1.0
    ay = (2.0 * math.pi * cy[:, None] * inv[None, :])[:, None, :].expand(gh, gw, q)
    ax = (2.0 * math.pi * cx[:, None] * inv[None, :])[None, :, :].expand(gh, gw, q)
    a = torch.cat([ay, ax], dim=-1).reshape(gh * gw, 2 * q)
    return torch.cos(a).to(torch.float32), torch.sin(a).to(torch.float32)


def split_head_weights(weights):
    """(encoder weights, head weights): the head.* entries of a translated CLIP / SigLIP state_dict apart from the rest."""
    enc = {k: v for k, v in weights.items() if not k.startswith("head.")}
    return enc, {k: v for k, v in weights.items() if k.startswith("head.")}


def expected_weight_shapes(cfg) -> "dict[str, tuple]":
    """Names and PyTorch shapes a config expects (same list vdr_weight_name enumerates)."""
    D, Fh = cfg.dim, cfg.mlp_hidden
    s = {}
    if cfg.patch:
        s["patch_embed.proj.weight"] = (D, cfg.in_chans, cfg.patch, cfg.patch)
        s["patch_embed.proj.bias"] = (D,)
    if cfg.has_cls:
        s["cls_token"] = (1, 1, D)
    if getattr(cfg, "n_register", 0):
        s["register_tokens"] = (1, cfg.n_register, D)
    if cfg.has_pos:  # (register tokens carry no position)
        s["pos_embed"] = (1, cfg.n_patches + (1 if cfg.has_cls else 0), D)
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
        if cfg.act == "swiglu":  # ("gelu", "quick_gelu", "gelu_tanh": fc1 / fc2)
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


# ---- SAM prompt encoder / mask decoder: the two spellings of one set of tensors -----------------------------------------
# (segment_anything, transformers.SamModel); "{i}" is a transformer layer, "{m}" one of the 4 point embeddings / hypernetworks.
# A name is spelled the same in both unless it matches a row here.  The hypernetwork and IoU-head MLPs are the one ambiguous
# spot: `layers.0` is the FIRST linear for segment_anything and the MIDDLE one for transformers (proj_in, layers.0, proj_out).
_SAM_DECODER_SPELLINGS = (
    ("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "shared_image_embedding.positional_embedding"),
    ("prompt_encoder.point_embeddings.{m}.", "prompt_encoder.point_embed.{m}."),
    ("prompt_encoder.mask_downscaling.0.", "prompt_encoder.mask_embed.conv1."),
    ("prompt_encoder.mask_downscaling.1.", "prompt_encoder.mask_embed.layer_norm1."),
    ("prompt_encoder.mask_downscaling.3.", "prompt_encoder.mask_embed.conv2."),
    ("prompt_encoder.mask_downscaling.4.", "prompt_encoder.mask_embed.layer_norm2."),
    ("prompt_encoder.mask_downscaling.6.", "prompt_encoder.mask_embed.conv3."),
    ("mask_decoder.transformer.layers.{i}.norm1.", "mask_decoder.transformer.layers.{i}.layer_norm1."),
    ("mask_decoder.transformer.layers.{i}.norm2.", "mask_decoder.transformer.layers.{i}.layer_norm2."),
    ("mask_decoder.transformer.layers.{i}.norm3.", "mask_decoder.transformer.layers.{i}.layer_norm3."),
    ("mask_decoder.transformer.layers.{i}.norm4.", "mask_decoder.transformer.layers.{i}.layer_norm4."),
    ("mask_decoder.transformer.norm_final_attn.", "mask_decoder.transformer.layer_norm_final_attn."),
    ("mask_decoder.output_upscaling.0.", "mask_decoder.upscale_conv1."),
    ("mask_decoder.output_upscaling.1.", "mask_decoder.upscale_layer_norm."),
    ("mask_decoder.output_upscaling.3.", "mask_decoder.upscale_conv2."),
    ("mask_decoder.output_hypernetworks_mlps.{m}.layers.0.", "mask_decoder.output_hypernetworks_mlps.{m}.proj_in."),
    ("mask_decoder.output_hypernetworks_mlps.{m}.layers.1.", "mask_decoder.output_hypernetworks_mlps.{m}.layers.0."),
    ("mask_decoder.output_hypernetworks_mlps.{m}.layers.2.", "mask_decoder.output_hypernetworks_mlps.{m}.proj_out."),
    ("mask_decoder.iou_prediction_head.layers.0.", "mask_decoder.iou_prediction_head.proj_in."),
    ("mask_decoder.iou_prediction_head.layers.1.", "mask_decoder.iou_prediction_head.layers.0."),
    ("mask_decoder.iou_prediction_head.layers.2.", "mask_decoder.iou_prediction_head.proj_out."),
)
SAM_DECODER_PREFIXES = ("prompt_encoder.", "mask_decoder.", "shared_image_embedding.")


def sam_decoder_name(name: str, to: str) -> str:
    """One prompt-encoder / mask-decoder tensor name in the other spelling: to="hf" takes a segment_anything name to
    transformers.SamModel's, to="sa" the reverse.  Names the two libraries share come back unchanged."""
    import re
    if to not in ("hf", "sa"):
        raise ValueError(f"to must be 'hf' or 'sa', got {to!r}")
    for sa, hf in _SAM_DECODER_SPELLINGS:
        src, dst = (sa, hf) if to == "hf" else (hf, sa)
        pat = "^" + re.escape(src).replace(r"\{i\}", r"(?P<i>\d+)").replace(r"\{m\}", r"(?P<m>\d+)")
        mt = re.match(pat, name)
        if mt:
            return dst.format(**mt.groupdict()) + name[mt.end():]
    return name


def split_sam_decoder_weights(sd):
    """A SAM state dict in either spelling -> (everything else, the prompt-encoder / mask-decoder tensors under their
    segment_anything names as fp32, or None when the checkpoint has none).  transformers' spelling is recognised by a name
    only it uses (proj_in, upscale_conv1, shared_image_embedding)."""
    dec = {k: v for k, v in sd.items() if k.startswith(SAM_DECODER_PREFIXES)}
    if not dec:
        return sd, None
    rest = {k: v for k, v in sd.items() if k not in dec}
    hf = any(".proj_in." in k or ".upscale_conv1." in k or k.startswith("shared_image_embedding.") for k in dec)
    out = {}
    for k, v in dec.items():
        if hf and k == "prompt_encoder.shared_embedding.positional_embedding":
            continue  # (tied to shared_image_embedding.positional_embedding)
        out[sam_decoder_name(k, "sa") if hf else k] = torch.as_tensor(v).detach().to(torch.float32).contiguous()
    return rest, out


_SAM_HF_ENCODER = (("patch_embed.projection.", "patch_embed.proj."), (".layer_norm1.", ".norm1."), (".layer_norm2.", ".norm2."),
                   (".mlp.lin1.", ".mlp.fc1."), (".mlp.lin2.", ".mlp.fc2."))
_SAM_HF_NECK = {"neck.conv1.": "neck.0.", "neck.layer_norm1.": "neck.1.", "neck.conv2.": "neck.2.", "neck.layer_norm2.": "neck.3."}


def from_sam_hf_vision_state_dict(sd):
    """The vision_encoder.* tensors of a transformers.SamModel / SamVisionModel state dict -> the canonical encoder names
    vdr_set_weight understands (layers.{i} -> blocks.{i}, layer_norm{1,2} -> norm{1,2}, mlp.lin{1,2} -> mlp.fc{1,2},
    patch_embed.projection -> patch_embed.proj, neck.conv1 / layer_norm1 / conv2 / layer_norm2 -> neck.0 .. neck.3); every
    other key is passed through."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("vision_encoder."):
            out[k] = v
            continue
        k = k[len("vision_encoder."):]
        if k.startswith("layers."):
            k = "blocks." + k[len("layers."):]
        for a, b in _SAM_HF_NECK.items():
            if k.startswith(a):
                k = b + k[len(a):]
        for a, b in _SAM_HF_ENCODER:
            k = k.replace(a, b)
        out[k] = v
    return out
