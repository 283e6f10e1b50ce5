"""Pure-torch fp32 restatement of the transformers CLIP / SigLIP vision towers and their heads (TEST HELPER).

The oracle (oracle/vit_oracle.py) knows erf-GELU and SwiGLU; the language-supervised towers use QuickGELU and
tanh-GELU, a pre_layrnorm (CLIP), a projection (CLIP) and an attention-pooling head (SigLIP).  This module restates them
on the oracle's pieces (patch_embed, assemble_tokens, layer_norm, attention) over the canonical weight names
(vdr.weights.from_clip_vision_state_dict / from_siglip_vision_state_dict) and is pinned to transformers itself by
tests/golden/clip_hf_tiny.npz / siglip_hf_tiny.npz (tests/test_clip_cpu.py: <= 2e-5 max-abs).

emulate=True rounds to bf16 where the HIP path stores bf16 (as vit_oracle's emulate_bf16=True does).
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_oracle as vo

ACTS = {
    "gelu": vo.gelu_erf,
    "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x),       # transformers QuickGELUActivation
    "gelu_tanh": lambda x: F.gelu(x, approximate="tanh"),        # transformers "gelu_pytorch_tanh"
}


def tiny_cfg(g, family: str) -> vo.VitCfg:
    """VitCfg of a *_hf_tiny.npz golden (family: "clip" | "siglip")"""
    clip = family == "clip"
    return vo.VitCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]),
                     act="quick_gelu" if clip else "gelu_tanh", has_cls=clip, input_ln=clip, ln_eps=float(g["ln_eps"]))


def golden_state_dict(g) -> dict:
    """the transformers state_dict a golden holds under sd.<key>"""
    return {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}


def tiny_model(golden_dir, family, **kw):
    """(golden, VitCfg, translated weights, model) of a tiny golden, loaded through load_model's key detection"""
    import vdr
    import handle_configs as hc
    g = np.load(os.path.join(golden_dir, family + "_hf_tiny.npz"), allow_pickle=False)
    cfg = tiny_cfg(g, family)
    sd = golden_state_dict(g)
    name = f"_{family}_tiny_test"
    vdr.ARCHS[name] = hc.vit_config(cfg)
    try:
        model = vdr.load_model(name, weights=sd, **kw)  # transformers keys: translated on the way in
    finally:
        del vdr.ARCHS[name]
    from vdr import weights as W
    w = (W.from_clip_vision_state_dict if family == "clip" else W.from_siglip_vision_state_dict)(sd)
    return g, cfg, w, model


def make_weights(cfg: vo.VitCfg, family: str, seed: int, scale: float = 0.02, proj: int = 512) -> dict:
    """Seeded weights of a tower (the oracle's recipe) plus its head under head.* keys."""
    w = vo.make_weights(cfg, seed=seed, scale=scale)
    D, Fh = cfg.dim, cfg.mlp_hidden
    g = torch.Generator().manual_seed(seed + 1000)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    if family == "clip":
        w["head.visual_projection.weight"] = scale * rn(proj, D)
        return w
    w.update({"head.probe": 0.02 * rn(1, 1, D), "head.attention.in_proj_weight": scale * rn(3 * D, D),
              "head.attention.in_proj_bias": scale * rn(3 * D), "head.attention.out_proj.weight": scale * rn(D, D),
              "head.attention.out_proj.bias": scale * rn(D), "head.layernorm.weight": 1.0 + 0.1 * rn(D),
              "head.layernorm.bias": 0.1 * rn(D), "head.mlp.fc1.weight": scale * rn(Fh, D), "head.mlp.fc1.bias": scale * rn(Fh),
              "head.mlp.fc2.weight": scale * rn(D, Fh), "head.mlp.fc2.bias": scale * rn(D)})
    return w


def _r(x, emulate):
    return vo._r(x, emulate)


@torch.no_grad()
def tower(cfg: vo.VitCfg, w, images, emulate=False, want_attn=False):
    """[B, 3, H, W] -> dict: raw [B, N, D] (the stream after the last block, before the final norm), tokens (after it),
    layers (the raw stream after every block), attn (want_attn: softmax(q k^T / sqrt(dh)) of every block, [B, H, N, N]).
    H, W other than cfg.img: pos_embed resampled as transformers' interpolate_pos_encoding (bicubic, float64)."""
    from vdr.weights import interpolate_pos_embed
    act, eps, ncls = ACTS[cfg.act], cfg.ln_eps, 1 if cfg.has_cls else 0
    images = images.to(torch.float32)
    B, _, H, W = images.shape
    w = dict(w)
    if (H, W) != (cfg.img, cfg.img):
        w["pos_embed"] = interpolate_pos_embed(w["pos_embed"], (H // cfg.patch, W // cfg.patch), ncls)
    x = vo.assemble_tokens(cfg, w, vo.patch_embed(images, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], cfg.patch, emulate))
    if cfg.input_ln:
        x = vo.layer_norm(_r(x, emulate), w["input_norm.weight"], w["input_norm.bias"], eps)
    x = _r(x, emulate)
    layers, attn = [], []
    dh = cfg.dim // cfg.heads
    for i in range(cfg.layers):
        p = f"blocks.{i}."
        h = _r(vo.layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"], eps), emulate)
        if want_attn:
            qkv = _r(h @ _r(w[p + "attn.qkv.weight"], emulate).t() + w[p + "attn.qkv.bias"], emulate)
            q, k, _ = qkv.reshape(B, -1, 3, cfg.heads, dh).permute(2, 0, 3, 1, 4)
            attn.append(torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh)), dim=-1))
        x = _r(x + vo.attention(h, w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"], w[p + "attn.proj.weight"],
                                w[p + "attn.proj.bias"], cfg.heads, emulate), emulate)
        y = _r(vo.layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"], eps), emulate)
        u = _r(act(y @ _r(w[p + "mlp.fc1.weight"], emulate).t() + w[p + "mlp.fc1.bias"]), emulate)
        x = _r(x + u @ _r(w[p + "mlp.fc2.weight"], emulate).t() + w[p + "mlp.fc2.bias"], emulate)
        layers.append(x)
    return {"raw": x, "tokens": vo.layer_norm(x, w["norm.weight"], w["norm.bias"], eps), "layers": layers, "attn": attn}


@torch.no_grad()
def pool_attention(q, k, v, heads):
    """one-query attention: q [D], k / v [B, n, D] -> [B, D] (fp32 softmax, maximum subtracted)"""
    B, n, D = k.shape
    dh = D // heads
    s = torch.einsum("hd,bnhd->bhn", q.reshape(heads, dh), k.reshape(B, n, heads, dh)) * (1.0 / math.sqrt(dh))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhn,bnhd->bhd", p, v.reshape(B, n, heads, dh)).reshape(B, D)


@torch.no_grad()
def clip_forward(cfg, w, images, emulate=False):
    """CLIPVisionModelWithProjection: last_hidden_state (encoder output, no post_layernorm), pooler_output
    (post_layernorm of the CLS row), image_embeds (visual_projection of it); plus the tower's dict entries."""
    t = tower(cfg, w, images, emulate)
    pooled = t["tokens"][:, 0]
    out = dict(t, last_hidden_state=t["raw"], pooler_output=pooled)
    if "head.visual_projection.weight" in w:
        out["image_embeds"] = _r(_r(pooled, emulate) @ _r(w["head.visual_projection.weight"], emulate).t(), emulate)
    return out


@torch.no_grad()
def siglip_forward(cfg, w, images, emulate=False):
    """SiglipVisionModel: last_hidden_state (after post_layernorm), pooler_output (SiglipMultiheadAttentionPoolingHead:
    nn.MultiheadAttention with the probe as the only query, then x + mlp(layernorm(x)))."""
    t = tower(cfg, w, images, emulate)
    D, eps = cfg.dim, cfg.ln_eps
    tok = _r(t["tokens"], emulate)
    W, b = w["head.attention.in_proj_weight"], w["head.attention.in_proj_bias"]
    q = w["head.probe"].reshape(1, D) @ W[:D].t() + b[:D]
    kv = _r(tok @ _r(W[D:], emulate).t() + b[D:], emulate)
    o = _r(pool_attention(q.reshape(D), kv[..., :D], kv[..., D:], cfg.heads), emulate)
    a = _r(o @ _r(w["head.attention.out_proj.weight"], emulate).t() + w["head.attention.out_proj.bias"], emulate)
    h = _r(vo.layer_norm(a, w["head.layernorm.weight"], w["head.layernorm.bias"], eps), emulate)
    u = _r(ACTS["gelu_tanh"](h @ _r(w["head.mlp.fc1.weight"], emulate).t() + w["head.mlp.fc1.bias"]), emulate)
    y = _r(a + u @ _r(w["head.mlp.fc2.weight"], emulate).t() + w["head.mlp.fc2.bias"], emulate)
    return dict(t, last_hidden_state=t["tokens"], pooler_output=y)


# ---- the device activation formulas, restated in fp32 on the CPU (csrc/vdr_dev.h: x_sigmoid, quick_gelu, gelu_tanh) ----
LOG2E = 1.44269504088896341


def device_activation_fp32(x: torch.Tensor, kind: str) -> torch.Tensor:
    """x fp32 -> x * (1 / (1 + exp2(e2))) with every step rounded to fp32 as the kernels do; exp2 and the reciprocal are
    torch's (correctly rounded to well under an ulp; the device's v_exp_f32 / v_rcp_f32 are good to 1 ulp)."""
    f = torch.float32
    x = x.to(f)
    if kind == "quick_gelu":
        c = torch.tensor(-1.702, dtype=f) * torch.tensor(LOG2E, dtype=f)  # (the constant is folded in fp32: QGELU_E2)
        e2 = x * c
    elif kind == "gelu_tanh":
        a = torch.tensor(-2.0, dtype=f) * torch.tensor(0.7978845608028654, dtype=f) * torch.tensor(LOG2E, dtype=f)  # TGELU_E2A
        bb = a * torch.tensor(0.044715, dtype=f)                                                                        # TGELU_E2B
        x2 = x * x
        inner = torch.addcmul(a.double(), x2.double(), bb.double()).to(f)  # fmaf(x2, B, A): one rounding
        e2 = x * inner
    else:
        raise ValueError(kind)
    d = torch.exp2(e2.double()).to(f) + 1.0
    return x * (1.0 / d.double()).to(f)


def exact_activation_fp64(x: torch.Tensor, kind: str) -> torch.Tensor:
    """float64 reference of the two activations.  tanh-GELU is evaluated as x sigmoid(2 u), u = sqrt(2/pi) (x + 0.044715 x^3):
    the same function as torch's gelu(approximate="tanh") = 0.5 x (1 + tanh(u)), without its cancellation -- in float64
    1 + tanh(u) is exactly 0 below x = -6.6 and has lost half its digits by x = -5, while the true value is a perfectly
    normal small number a bf16 result must still match (tests/test_clip_cpu.py checks the two forms agree to float64's
    absolute resolution)."""
    x = x.double()
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x))


# ---- inputs of the activation-epilogue tests whose pre-activation is known exactly --------------------------------------
def epilogue_test_inputs(M, N, K, seed):
    """x [M, K] and W [N, K] (bf16-exact) on binary grids so coarse that every product and every partial sum of x W^T is
    exact in fp32 in ANY summation order: x in steps of 1/8 within [-2, 2], W in steps of 2^-7 with a width that gives the
    pre-activation a standard deviation of about 1.5 (what an fc1 sees); sums stay below 2^10 with a granularity of 2^-10,
    20 of fp32's 24 bits.  The bias is any fp32 number (0.3 N(0, 1)): the epilogue adds it with ONE rounding, acc + b.  So
    the fp32 pre-activation on the device IS fp32(float64 sum), and an activation-epilogue test measures the activation
    alone.  Returns (x, W, bias)."""
    g = torch.Generator().manual_seed(seed)
    s = max(2, int(round(1.5 / 1.22 * math.sqrt(3.0 / K) * 128)))
    x = torch.randint(-16, 17, (M, K), generator=g).float() / 8
    W = torch.randint(-s, s + 1, (N, K), generator=g).float() / 128
    b = 0.3 * torch.randn(N, generator=g)
    return x, W, b


def exact_preactivation(x, W, b):
    """fp32(x W^T + b) of epilogue_test_inputs, through float64 (on the tensors' device): the product sum is checked to be
    exactly an fp32 number, the bias add is the one rounding the epilogue performs"""
    acc64 = x.double() @ W.double().t()
    assert torch.equal(acc64.to(torch.float32).double(), acc64), "the designed product sums must be exact in fp32"
    return (acc64 + b.double()).to(torch.float32)


def bf16_ulp_distance(got_bf16, exact64):
    """|bit pattern distance| between bf16 values and the correctly rounded bf16 of float64 values (same sign assumed
    wherever it matters: a sign flip shows as a huge distance)"""
    want = exact64.to(torch.float32).to(torch.bfloat16)
    return (got_bf16.view(torch.int16).int() - want.view(torch.int16).int()).abs()
