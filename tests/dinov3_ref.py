"""Pure-torch fp32 restatement of DINOv3 (transformers DINOv3ViTModel) and DINOv2-with-registers (Dinov2WithRegistersModel /
hub dinov2_vit*14_reg) over the canonical weight names (TEST HELPER).

oracle.vit_oracle's VitCfg knows one prefix token and no rotary embedding; this module adds register tokens and the axial
2-D RoPE on the oracle's pieces (patch_embed, layer_norm, sdpa, mlp) and is pinned to transformers itself by
tests/golden/dinov3_hf_tiny.npz / dinov3_hf_gated_hd64.npz / dinov2reg_hf_tiny.npz (tests/test_dinov3_cpu.py: <= 2e-5
max-abs).

Tokens are [cls | R registers | n patches].  DINOv2-with-registers adds pos_embed [1, 1 + n, D] to [cls | patches] first
and inserts the registers after row 0; DINOv3 has no table and rotates q / k of the patch rows in every block.

emulate=True rounds to bf16 where the HIP path stores bf16 (as vit_oracle's emulate_bf16=True does): that includes the
bf16 qkv activation BEFORE the rotation and the bf16 q / k AFTER it, and the rotation follows vdr_op_rope2d's fp32
operation order (p1 = lo c, p2 = hi s, lo' = p1 - p2; p3 = hi c, p4 = lo s, hi' = p3 + p4, one rounding each).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import vit_oracle as vo


@dataclass
class RegCfg:
    """a vo.VitCfg plus what this family adds"""
    vit: vo.VitCfg
    n_register: int = 0
    rope: bool = False
    rope_theta: float = 100.0

    @property
    def n_prefix(self):
        return (1 if self.vit.has_cls else 0) + self.n_register


def golden_cfg(g, family: str) -> RegCfg:
    """RegCfg of a golden (family: "dinov3" | "dinov2reg")"""
    v3 = family == "dinov3"
    vit = vo.VitCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]),
                    act="swiglu" if int(g["gated"]) else "gelu", layerscale=True, has_pos=not v3, ln_eps=float(g["ln_eps"]))
    return RegCfg(vit, int(g["registers"]), v3, float(g["rope_theta"]) if v3 else 100.0)


def vdr_config(rc: RegCfg, **kw):
    """the vdr.VdrConfig of a RegCfg"""
    import vdr
    c = rc.vit
    return vdr.VdrConfig(img=c.img, patch=c.patch, dim=c.dim, heads=c.heads, layers=c.layers, mlp_hidden=c.mlp_hidden, act=c.act,
                         layerscale=c.layerscale, has_pos=c.has_pos, ln_eps=c.ln_eps, n_register=rc.n_register, rope=rc.rope,
                         rope_theta=rc.rope_theta, **kw)


def golden_state_dict(g) -> dict:
    """the transformers state_dict a golden holds under sd.<key>"""
    return {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}


def make_weights(rc: RegCfg, seed: int, scale: float = 0.02) -> dict:
    """Seeded weights (the oracle's recipe) plus register_tokens ~ 0.02 N from a PCG64 stream of their own."""
    w = vo.make_weights(rc.vit, seed=seed, scale=scale)
    if rc.n_register:
        z = np.random.Generator(np.random.PCG64([seed, 9001])).standard_normal(size=(1, rc.n_register, rc.vit.dim), dtype=np.float32)
        w["register_tokens"] = torch.from_numpy(0.02 * z)
    return w


def rope_table(grid, head_dim, theta):
    """(cos, sin) fp32 [gh*gw, head_dim/2]: float64 evaluation rounded once (vdr_op_rope2d_table's policy)"""
    from vdr.weights import rope2d_table
    return rope2d_table(grid, head_dim, theta)


def rotate(t, cos, sin):
    """t [..., n, dh] fp32, cos / sin [n, dh/2] fp32: the rotate_half rotation in vdr_op_rope2d's fp32 operation order"""
    half = t.shape[-1] // 2
    lo, hi = t[..., :half], t[..., half:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], dim=-1)


def assemble(rc: RegCfg, w, pe):
    """patch embeddings [B, n, D] -> [cls | registers | patches] with the family's positions"""
    c, B = rc.vit, pe.shape[0]
    x = torch.cat([w["cls_token"].reshape(1, 1, -1).expand(B, 1, -1), pe], dim=1) if c.has_cls else pe
    if c.has_pos:
        x = x + w["pos_embed"].reshape(1, x.shape[1], -1)
    if rc.n_register:
        reg = w["register_tokens"].reshape(1, rc.n_register, -1).expand(B, -1, -1)
        x = torch.cat([x[:, :1], reg, x[:, 1:]], dim=1)
    return x


@torch.no_grad()
def forward(rc: RegCfg, w, images, emulate=False, want_attn=False):
    """[B, 3, H, W] -> dict: raw [B, N, D] (the stream after the last block), tokens (after the final norm: transformers'
    last_hidden_state), cls (row 0), dense (rows P..), layers (the raw stream after every block), attn (want_attn:
    softmax(q k^T / sqrt(dh)) of every block from the rotated q / k, [B, H, N, N]).  H, W other than cfg.img: pos_embed
    resampled by vdr.weights.interpolate_pos_embed (bicubic, float64, no antialias); the RoPE table follows the grid."""
    from vdr.weights import interpolate_pos_embed
    c, r = rc.vit, vo._r
    eps, P, heads, dh = c.ln_eps, rc.n_prefix, c.heads, c.dim // c.heads
    images = images.to(torch.float32)
    B, _, H, W = images.shape
    grid = (H // c.patch, W // c.patch)
    w = dict(w)
    if c.has_pos and (H, W) != (c.img, c.img):
        w["pos_embed"] = interpolate_pos_embed(w["pos_embed"], grid, 1 if c.has_cls else 0)
    x = r(assemble(rc, w, vo.patch_embed(images, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], c.patch, emulate)), emulate)
    cos, sin = rope_table(grid, dh, rc.rope_theta) if rc.rope else (None, None)
    layers, attn = [], []
    for i in range(c.layers):
        p = f"blocks.{i}."
        g1 = w[p + "ls1.gamma"] if c.layerscale else 1.0
        g2 = w[p + "ls2.gamma"] if c.layerscale else 1.0
        h = r(vo.layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"], eps), emulate)
        qkv = r(h @ r(w[p + "attn.qkv.weight"], emulate).t() + w[p + "attn.qkv.bias"], emulate)
        q, k, v = qkv.reshape(B, -1, 3, heads, dh).permute(2, 0, 3, 1, 4)  # [B, H, N, dh]
        if rc.rope:
            q = torch.cat([q[:, :, :P], r(rotate(q[:, :, P:], cos, sin), emulate)], dim=2)
            k = torch.cat([k[:, :, :P], r(rotate(k[:, :, P:], cos, sin), emulate)], dim=2)
        if want_attn:
            attn.append(torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh)), dim=-1))
        o = vo.sdpa(q, k, v, emulate).transpose(1, 2).reshape(B, -1, c.dim)
        a = r(o, emulate) @ r(w[p + "attn.proj.weight"], emulate).t() + w[p + "attn.proj.bias"]
        x = r(x + g1 * a, emulate)
        y = r(vo.layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"], eps), emulate)
        x = r(x + g2 * vo.mlp(y, w, p + "mlp.", c.act, emulate), emulate)
        layers.append(x)
    tokens = vo.layer_norm(x, w["norm.weight"], w["norm.bias"], eps)
    return {"raw": x, "tokens": tokens, "cls": tokens[:, 0], "dense": tokens[:, P:], "layers": layers, "attn": attn}
