"""SAM's box-prompt encoder and mask decoder, restated (TEST HELPER, not collected).

* `decode(w, emb, boxes, cfg, mode)`: the definition in float64 (mode="f64"), or with a rounding to bf16 at every point where
  the device stores bf16 (mode="bf16": vdr/segment.py's composition, include/vdr.h "mask decoder ops").
* the weight recipe of the goldens (`draw_weights`): numpy.random.RandomState(seed), the frozen legacy stream, key by key in
  sorted order of the segment_anything names, every value rounded to a bf16-representable one; `weights_sha256` pins the bytes.
* op-level restatements with their entry-wise fp32 bounds (`cross_attention_ref`, `mask_upscale_ref`, `token_linear_ref`).
* the two spellings of the decoder's names come from vdr.weights (one table); `to_hf` spells a drawn dict transformers' way.

Parity of the definition is pinned against transformers.SamModel 5.15.0 (tests/golden/make_golden_sam_decoder.py):
segment_anything itself is not installed where the goldens are made."""
import hashlib
import math

import numpy as np
import torch

U32 = 2.0 ** -24   # unit roundoff of fp32
U16 = 2.0 ** -8    # ... of bf16 (8 significant bits)
# the device GELU (csrc/vdr_dev.h gelu_erf; pinned by the GELU-epilogue tests of tests/test_ops_gpu.py and the designed
# epilogue cases of tests/core_ops_designs.py): absolute error of the degree-6 polynomial form against the exact erf GELU
GELU_ABS_ERR = 4.8e-6


def bf16(x):
    """fp32 -> bf16 -> float64, round to nearest even: the device's one rounding of an fp32 value it stores as bf16"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32(x):
    return x.to(torch.float32).to(torch.float64)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- shapes, weights ---------------------------------------------------------------------------------------------------
def decoder_shapes(mlp_dim=2048, C=256, depth=2):
    """segment_anything name -> shape of every tensor the box-prompt path reads"""
    s = {"prompt_encoder.pe_layer.positional_encoding_gaussian_matrix": (2, C // 2),
         "prompt_encoder.no_mask_embed.weight": (1, C),
         "mask_decoder.iou_token.weight": (1, C), "mask_decoder.mask_tokens.weight": (4, C)}
    for i in range(4):
        s[f"prompt_encoder.point_embeddings.{i}.weight"] = (1, C)

    def attn(p, inner):
        for n in ("q_proj", "k_proj", "v_proj"):
            s[p + n + ".weight"], s[p + n + ".bias"] = (inner, C), (inner,)
        s[p + "out_proj.weight"], s[p + "out_proj.bias"] = (C, inner), (C,)

    def ln(p, d=C):
        s[p + ".weight"], s[p + ".bias"] = (d,), (d,)
    for i in range(depth):
        p = f"mask_decoder.transformer.layers.{i}."
        attn(p + "self_attn.", C)
        attn(p + "cross_attn_token_to_image.", C // 2)
        attn(p + "cross_attn_image_to_token.", C // 2)
        s[p + "mlp.lin1.weight"], s[p + "mlp.lin1.bias"] = (mlp_dim, C), (mlp_dim,)
        s[p + "mlp.lin2.weight"], s[p + "mlp.lin2.bias"] = (C, mlp_dim), (C,)
        for j in range(1, 5):
            ln(p + f"norm{j}")
    attn("mask_decoder.transformer.final_attn_token_to_image.", C // 2)
    ln("mask_decoder.transformer.norm_final_attn")
    s["mask_decoder.output_upscaling.0.weight"], s["mask_decoder.output_upscaling.0.bias"] = (C, C // 4, 2, 2), (C // 4,)
    ln("mask_decoder.output_upscaling.1", C // 4)
    s["mask_decoder.output_upscaling.3.weight"], s["mask_decoder.output_upscaling.3.bias"] = (C // 4, C // 8, 2, 2), (C // 8,)
    for m in range(4):
        p = f"mask_decoder.output_hypernetworks_mlps.{m}.layers."
        for j, (o, i_) in enumerate(((C, C), (C, C), (C // 8, C))):
            s[p + f"{j}.weight"], s[p + f"{j}.bias"] = (o, i_), (o,)
    p = "mask_decoder.iou_prediction_head.layers."
    for j, (o, i_) in enumerate(((C, C), (C, C), (4, C))):
        s[p + f"{j}.weight"], s[p + f"{j}.bias"] = (o, i_), (o,)
    return s


def draw_weights(seed, mlp_dim=128, gain=1.0):
    """The goldens' decoder weights (segment_anything names, fp32 tensors holding bf16-representable values).  Linear and
    transposed-convolution weights are N(0, 1) / sqrt(fan_in) (x 2 for the attention projections and the last hypernetwork
    layer, so that the softmaxes are not flat and the logits have spread: the generator asserts the spread), biases and
    embeddings N(0, 1) x 0.1 (tokens, corner embeddings: x 1), LayerNorm gains 1 + 0.1 N(0, 1).  `gain` scales the last
    hypernetwork layer once more."""
    rs = np.random.RandomState(seed)
    out = {}
    for k, shp in sorted(decoder_shapes(mlp_dim).items()):
        a = rs.standard_normal(shp)
        if "gaussian_matrix" in k:
            pass  # scale 1, as segment_anything draws it
        elif ".norm" in k or "output_upscaling.1." in k:
            a = (1.0 + 0.1 * a) if k.endswith(".weight") else 0.1 * a
        elif k.endswith(".bias"):
            a = 0.1 * a
        elif len(shp) == 4:
            a = a / math.sqrt(shp[0])
        elif "_proj." in k:
            a = 2.0 * a / math.sqrt(shp[1])
        elif "hypernetworks_mlps" in k and ".layers.2." in k:
            a = 2.0 * gain * a / math.sqrt(shp[1])
        elif "layers." in k or "lin" in k:
            a = a / math.sqrt(shp[1])
        # (tokens and embeddings: N(0, 1))
        out[k] = torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).to(torch.float32)
    return out


def weights_sha256(w):
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(w[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def to_hf(w):
    """a segment_anything-spelled decoder dict in transformers.SamModel's spelling (vdr.weights' table)"""
    from vdr.weights import sam_decoder_name
    out = {sam_decoder_name(k, "hf"): v for k, v in w.items()}
    out["prompt_encoder.shared_embedding.positional_embedding"] = out["shared_image_embedding.positional_embedding"]
    return out


# ---- the definition ----------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, g, img, mlp_dim=2048, ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6):
        self.g, self.img, self.mlp_dim = g, img, mlp_dim
        self.ln_eps, self.final_ln_eps, self.ln2d_eps = ln_eps, final_ln_eps, ln2d_eps


HF_EPS = dict(ln_eps=1e-6, final_ln_eps=1e-5, ln2d_eps=1e-6)   # what transformers 5.15.0 applies (its config's layer_norm_eps)
SA_EPS = dict(ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6)   # segment_anything: nn.LayerNorm's default, LayerNorm2d's 1e-6


def fourier_pe(coords01, gauss):
    """coords in [0, 1] [..., 2] (x, y) -> [..., 256]"""
    c = (2.0 * coords01 - 1.0) @ gauss.double()
    c = 2.0 * math.pi * c
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


def dense_pe(g, gauss):
    t = (torch.arange(g, dtype=torch.float64) + 0.5) / g
    yy, xx = torch.meshgrid(t, t, indexing="ij")
    return fourier_pe(torch.stack([xx, yy], dim=-1), gauss).reshape(g * g, -1)   # [n, 256], cell = y * g + x


def box_tokens(boxes, img, w):
    """boxes [B, nb, 4] pixels -> [B*nb, 2, 256]"""
    c = (boxes.double().reshape(-1, 2, 2) + 0.5) / float(img)
    pe = fourier_pe(c, w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"])
    pe[:, 0] += w["prompt_encoder.point_embeddings.2.weight"][0].double()
    pe[:, 1] += w["prompt_encoder.point_embeddings.3.weight"][0].double()
    return pe


def _ln(x, w, p, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w[p + ".weight"].double() + w[p + ".bias"].double()


def _lin(x, w, p):
    return x @ w[p + ".weight"].double().T + w[p + ".bias"].double()


def _attend(q, k, v, heads):
    P, tq, D = q.shape
    dh = D // heads
    qh, kh, vh = (t.reshape(P, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    a = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (a @ vh).transpose(1, 2).reshape(P, tq, D)


def decode(w, emb, boxes, cfg, mode="f64"):
    """w: segment_anything-spelled weights; emb [B, 256, g, g]; boxes [B, nb, 4] -> (low_res_logits [B, nb, 4, 4g, 4g],
    iou [B, nb, 4]) as float64, all four mask tokens (multimask=False is token 0, True tokens 1..3)."""
    r = bf16 if mode == "bf16" else (lambda t: t)
    B, C, g, _ = emb.shape
    nb = boxes.shape[1]
    P, n = B * nb, g * g
    gauss = w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"]
    kpe = dense_pe(g, gauss)
    if mode == "bf16":
        kpe = f32(kpe)
    sparse = box_tokens(boxes, cfg.img, w)
    fixed = torch.cat([w["mask_decoder.iou_token.weight"], w["mask_decoder.mask_tokens.weight"]], 0).double()
    tok = r(torch.cat([fixed[None].expand(P, -1, -1), sparse], dim=1))   # [P, 7, 256]
    pe = tok.clone()
    keys = emb.double().reshape(B, C, n).transpose(1, 2) + w["prompt_encoder.no_mask_embed.weight"].double()
    keys = r(keys.repeat_interleave(nb, dim=0))                        # [P, n, 256]
    T = "mask_decoder.transformer."

    def t2i(p, tok, keys, ln, eps):
        q = r(_lin(r(tok + pe), w, p + "q_proj"))
        if mode == "bf16":  # the device adds the fp32 table kpe Wk^T + bk to the bf16 rows keys Wk^T
            k = r(keys @ w[p + "k_proj.weight"].double().T) + f32(_lin(kpe, w, p + "k_proj"))
        else:
            k = _lin(keys + kpe, w, p + "k_proj")
        v = r(_lin(keys, w, p + "v_proj"))
        a = r(_attend(q, k, v, 8))
        return r(_ln(r(tok + _lin(a, w, p + "out_proj")), w, ln, eps))

    for i in range(2):
        p = T + f"layers.{i}."
        if i == 0:
            a = r(_attend(r(_lin(tok, w, p + "self_attn.q_proj")), r(_lin(tok, w, p + "self_attn.k_proj")),
                          r(_lin(tok, w, p + "self_attn.v_proj")), 8))
            tok = r(_lin(a, w, p + "self_attn.out_proj"))
        else:
            x = r(tok + pe)
            a = r(_attend(r(_lin(x, w, p + "self_attn.q_proj")), r(_lin(x, w, p + "self_attn.k_proj")),
                          r(_lin(tok, w, p + "self_attn.v_proj")), 8))
            tok = r(tok + _lin(a, w, p + "self_attn.out_proj"))
        tok = r(_ln(tok, w, p + "norm1", cfg.ln_eps))
        tok = t2i(p + "cross_attn_token_to_image.", tok, keys, p + "norm2", cfg.ln_eps)
        h = r(torch.relu(_lin(tok, w, p + "mlp.lin1")))
        tok = r(_ln(r(tok + _lin(h, w, p + "mlp.lin2")), w, p + "norm3", cfg.ln_eps))
        q2 = p + "cross_attn_image_to_token."
        if mode == "bf16":
            q = r(keys @ w[q2 + "q_proj.weight"].double().T) + f32(_lin(kpe, w, q2 + "q_proj"))
        else:
            q = _lin(keys + kpe, w, q2 + "q_proj")
        k = r(_lin(r(tok + pe), w, q2 + "k_proj"))
        v = r(_lin(tok, w, q2 + "v_proj"))
        a = r(_attend(q, k, v, 8))
        keys = r(_ln(r(keys + _lin(a, w, q2 + "out_proj")), w, p + "norm4", cfg.ln_eps))
    tok = t2i(T + "final_attn_token_to_image.", tok, keys, T + "norm_final_attn", cfg.final_ln_eps)

    U = "mask_decoder.output_upscaling."
    W1 = w[U + "0.weight"].double()                                     # [256, 64, 2, 2]
    up = torch.einsum("pnc,cods->pndso", keys, W1) + w[U + "0.bias"].double()   # [P, n, dy, dx, 64]
    up = r(up)
    up = r(_ln(up, w, U + "1", cfg.ln2d_eps))
    up = r(gelu(up))
    W2 = w[U + "3.weight"].double()                                     # [64, 32, 2, 2]
    u2 = gelu(torch.einsum("pndsc,coet->pndseto", up, W2) + w[U + "3.bias"].double())   # [P, n, dy1, dx1, dy2, dx2, 32]
    hyper = []
    for m in range(4):
        p = f"mask_decoder.output_hypernetworks_mlps.{m}.layers."
        x = tok[:, 1 + m]
        x = r(torch.relu(_lin(x, w, p + "0")))
        x = r(torch.relu(_lin(x, w, p + "1")))
        hyper.append(_lin(x, w, p + "2"))
    hyper = torch.stack(hyper, dim=1)                                   # [P, 4, 32]
    if mode == "bf16":
        hyper = f32(hyper)
    lg = torch.einsum("pmo,pndseto->pmndset", hyper, u2)                # [P, 4, n, dy1, dx1, dy2, dx2]
    lg = lg.reshape(P, 4, g, g, 2, 2, 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(P, 4, 4 * g, 4 * g)
    p = "mask_decoder.iou_prediction_head.layers."
    x = tok[:, 0]
    x = r(torch.relu(_lin(x, w, p + "0")))
    x = r(torch.relu(_lin(x, w, p + "1")))
    iou = _lin(x, w, p + "2")
    return lg.reshape(B, nb, 4, 4 * g, 4 * g), iou.reshape(B, nb, 4)


# ---- op-level restatements and their fp32 bounds -----------------------------------------------------------------------
def cross_attention_ref(q, k, v, P, tq, tk, heads, dh, q_add=None, k_add=None):
    """float64 from the bf16 / fp32 operands -> (out [P*tq, H*dh] float64 before the rounding to bf16, bound): `bound` is
    the entry-wise fp32 error of ANY summation order of the device's kind (include/vdr.h): with u = 2^-24,
      |dt_ij| <= E_i = (dh + 6) u c max_j sum_d |Q_id K_jd|          (fma chain or tree, the table's addition, t = s c)
      p_j carries a relative error rho_i = ln2 (2 E_i + 3 u R_i) + 3 (tk + 16) u, R_i = max_j t_ij - min_j t_ij
                                           (v_exp_f32 to 1 ulp, the rescaling products, one fma per step and merge)
      |out - exact| <= 2 rho_i sum_j p_j |v_jd| / L + 2 u |out|      (numerator and denominator, the division).
    The device's bf16 output then lies between bf16(exact - bound) and bf16(exact + bound) (rounding is monotone)."""
    HD = heads * dh
    Q = q.double().reshape(P, tq, heads, dh)
    K = k.double().reshape(P, tk, heads, dh)
    V = v.double().reshape(P, tk, heads, dh)
    if q_add is not None:
        Q = Q + q_add.double().reshape(1, tq, heads, dh)
    if k_add is not None:
        K = K + k_add.double().reshape(1, tk, heads, dh)
    c = math.log2(math.e) / math.sqrt(dh)
    t = torch.einsum("pihd,pjhd->phij", Q, K) * c
    tabs = torch.einsum("pihd,pjhd->phij", Q.abs(), K.abs()) * c
    E = (dh + 6) * U32 * tabs.amax(-1)                                  # [P, H, tq]
    R = t.amax(-1) - t.amin(-1)
    rho = math.log(2.0) * (2 * E + 3 * U32 * R) + 3 * (tk + 16) * U32
    pr = torch.exp2(t - t.amax(-1, keepdim=True))
    L = pr.sum(-1)
    out = torch.einsum("phij,pjhd->pihd", pr, V) / L.permute(0, 2, 1)[..., None]
    mag = torch.einsum("phij,pjhd->pihd", pr, V.abs()) / L.permute(0, 2, 1)[..., None]
    bound = 2 * rho.permute(0, 2, 1)[..., None] * mag + 2 * U32 * out.abs()
    return out.reshape(P * tq, HD), bound.reshape(P * tq, HD)


def within_bf16_of(got, exact, bound):
    """got (bf16 tensor) lies in [bf16(exact - bound), bf16(exact + bound)]"""
    g = got.double().cpu()
    return bool(((g >= bf16(exact - bound)) & (g <= bf16(exact + bound))).all())


def token_linear_ref(x, W, bias=None, x_add=None, resid=None, relu=False, groups=1):
    """float64: x [M, K], W [groups, N, K]; returns (y float64 before the output rounding, bound): the fma chain over K
    obeys |dy| <= (K + 3) u (sum_k |x_k W_nk| + |b| + |resid|)."""
    X = x.double()
    if x_add is not None:
        X = bf16(X + x_add.double())
    M = X.shape[0]
    Wd = W.double().reshape(groups, -1, X.shape[1])
    gi = torch.arange(M) % groups
    y = torch.einsum("mk,mnk->mn", X, Wd[gi])
    mag = torch.einsum("mk,mnk->mn", X.abs(), Wd[gi].abs())
    if bias is not None:
        b = bias.double().reshape(groups, -1)[gi]
        y, mag = y + b, mag + b.abs()
    if relu:
        y = torch.relu(y)
    if resid is not None:
        y, mag = y + resid.double(), mag + resid.double().abs()
    return y, (X.shape[1] + 3) * U32 * mag


def mask_upscale_ref(x, W, bias, hyper, P, g, gelu_in):
    """float64 restatement of vdr_op_mask_upscale -> (logits [P, 4, 4g, 4g], bound).  Bound, entry-wise:
      a_k = bf16(gelu(x_k)): exact when gelu_in = 0.  Else the device rounds its polynomial's value, which is within
           GELU_ABS_ERR of gelu(x_k): the same bf16 value (da_k = 0) unless gelu(x_k) lies within 2 GELU_ABS_ERR of a rounding
           tie of bf16, where the other neighbour is allowed (da_k = one bf16 ulp at that value)
      pre-activation: |dz_c| <= 65 u sum_k |a_k W_ck| + u |z_c| + sum_k |W_ck| |da_k|     (fp32 MFMA accumulation, any order)
      u_c = gelu(z_c): |du_c| <= 1.13 |dz_c| + GELU_ABS_ERR + 4 u |u_c|                    (|gelu'| <= 1.13)
      logit: sum_c |hyper_c| |du_c| + 34 u sum_c |hyper_c u_c|                             (two fma chains and one addition)."""
    n = g * g
    X = x.double().reshape(P, n, 2, 2, 64)
    if gelu_in:
        y = gelu(X)
        a = bf16(y)
        ulp = torch.exp2(torch.floor(torch.log2(torch.minimum(a.abs(), y.abs()).clamp_min(2.0 ** -120))) - 7.0)   # spacing of bf16 on y's side of a
        near_tie = (0.5 * ulp - (y - a).abs()) <= 2.0 * GELU_ABS_ERR
        da = torch.where(near_tie, 2.0 * ulp, torch.zeros_like(y))   # (2 ulp: across a power of two the spacing doubles)
    else:
        a, da = X, torch.zeros_like(X)
    Wd = W.double().reshape(2, 2, 32, 64)                               # [dy2, dx2, c, k]
    z = torch.einsum("pndsk,etck->pndsetc", a, Wd) + bias.double()
    dz = 65 * U32 * torch.einsum("pndsk,etck->pndsetc", a.abs(), Wd.abs()) + U32 * z.abs() \
        + torch.einsum("pndsk,etck->pndsetc", da, Wd.abs())
    u = gelu(z)
    du = 1.13 * dz + GELU_ABS_ERR + 4 * U32 * u.abs()
    H = hyper.double()
    lg = torch.einsum("pmc,pndsetc->pmndset", H, u)
    bd = torch.einsum("pmc,pndsetc->pmndset", H.abs(), du) + 34 * U32 * torch.einsum("pmc,pndsetc->pmndset", H.abs(), u.abs())

    def scatter(t):
        return t.reshape(P, 4, g, g, 2, 2, 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(P, 4, 4 * g, 4 * g)
    return scatter(lg), scatter(bd)


# ---- the goldens ---------------------------------------------------------------------------------------------------------
def golden_case(golden_dir, tag):
    """tests/golden/sam_hf_decoder_<tag>.npz -> dict: the arrays as tensors, cfg (transformers' eps), the drawn decoder weights
    (SHA-256 checked before anything else), all4 / iou4 = the four mask tokens' outputs [B, nb, 4, ...] in token order."""
    import os
    z = np.load(os.path.join(golden_dir, f"sam_hf_decoder_{tag}.npz"), allow_pickle=False)
    w = draw_weights(int(z["dseed"]), int(z["mlp_dim"]))
    assert weights_sha256(w) == str(z["sha256"]), "the weight recipe no longer draws the bytes the golden was made with"
    c = {k: torch.from_numpy(z[k]) for k in ("image", "emb", "boxes", "pred_masks_multi", "iou_multi", "pred_masks_single", "iou_single")}
    c["weights"] = w
    c["cfg"] = Cfg(int(z["g"]), int(z["img"]), int(z["mlp_dim"]), float(z["ln_eps"]), float(z["final_ln_eps"]), float(z["ln2d_eps"]))
    c["eps"] = dict(ln_eps=float(z["ln_eps"]), final_ln_eps=float(z["final_ln_eps"]), ln2d_eps=float(z["ln2d_eps"]))
    c["all4"] = torch.cat([c["pred_masks_single"], c["pred_masks_multi"]], dim=2).double()
    c["iou4"] = torch.cat([c["iou_single"], c["iou_multi"]], dim=2).double()
    for k in ("f64_diff", "bf16_diff", "whole_diff", "enc_effect"):
        c[k] = tuple(float(v) for v in z[k])   # (relative L2, worst absolute difference, worst IoU-head difference)
    c["wseed"], c["xseed"] = int(z["wseed"]), int(z["xseed"])
    return c


def diffs(lg, iou, ref_lg, ref_iou):
    d = lg.double().cpu() - ref_lg.double()
    return float(d.norm() / ref_lg.double().norm()), float(d.abs().max()), float((iou.double().cpu() - ref_iou.double()).abs().max())


def encoder_to_hf(w):
    """canonical SAM encoder weights (oracle/sam_oracle.py's names) in transformers.SamModel's spelling"""
    out = {}
    for k, v in w.items():
        k = k.replace("patch_embed.proj.", "patch_embed.projection.").replace(".norm1.", ".layer_norm1.").replace(".norm2.", ".layer_norm2.")
        k = k.replace(".mlp.fc1.", ".mlp.lin1.").replace(".mlp.fc2.", ".mlp.lin2.")
        for a, b in (("neck.0.", "neck.conv1."), ("neck.1.", "neck.layer_norm1."), ("neck.2.", "neck.conv2."), ("neck.3.", "neck.layer_norm2.")):
            if k.startswith(a):
                k = b + k[len(a):]
        if k.startswith("blocks."):
            k = "layers." + k[len("blocks."):]
        out["vision_encoder." + k] = v
    return out
