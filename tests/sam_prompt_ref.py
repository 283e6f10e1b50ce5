"""SAM's point and mask prompts, restated (TEST HELPER, not collected).  Builds on sam_decoder_ref (the box-prompt decode).

* `draw_prompt_weights(seed)`: the 11 tensors the box path does not read (not_a_point_embed, mask_downscaling.*), from a
  numpy.random.RandomState of their own -- sam_decoder_ref.draw_weights and its SHA-256 are untouched.
* `sparse_tokens`: segment_anything's token rows [np points; one padding point if there is no box; 2 box corners if there is one],
  with transformers' label rules (1 / 0: pe + point_embeddings[label]; -1: not_a_point_embed; -10: zeros; else pe alone).
* `mask_dense`: mask_downscaling in float64.  `decode`: the whole decode at any T, float64 or bf16-rounding mode: it is
  sam_decoder_ref.decode with the sparse rows and the keys' additive term exchanged (the rest of the decoder does not depend on
  the prompt kind).
* `mask_embed_ref`: vdr_op_mask_embed in float64 with its entry-wise fp32 bound.  `mask_box_ref`: vdr_op_mask_box in torch.
"""
import math
import os

import numpy as np
import torch

import sam_decoder_ref as R

U32 = R.U32
MD = "prompt_encoder.mask_downscaling."


def prompt_shapes(C=256):
    return {"prompt_encoder.not_a_point_embed.weight": (1, C),
            MD + "0.weight": (4, 1, 2, 2), MD + "0.bias": (4,), MD + "1.weight": (4,), MD + "1.bias": (4,),
            MD + "3.weight": (16, 4, 2, 2), MD + "3.bias": (16,), MD + "4.weight": (16,), MD + "4.bias": (16,),
            MD + "6.weight": (C, 16, 1, 1), MD + "6.bias": (C,)}


def draw_prompt_weights(seed):
    """N(0, 1) / sqrt(fan_in) for the convolutions (x 2 for the last one, so that the mask prompt moves the keys), biases 0.1 N,
    LayerNorm gains 1 + 0.1 N, the embedding N(0, 1); every value bf16-representable, as the decoder's."""
    rs = np.random.RandomState(seed)
    out = {}
    for k, shp in sorted(prompt_shapes().items()):
        a = rs.standard_normal(shp)
        if k.endswith(".bias"):
            a = 0.1 * a
        elif len(shp) == 4:
            a = (2.0 if ".6." in k else 1.0) * a / math.sqrt(shp[1] * shp[2] * shp[3])
        elif len(shp) == 1:
            a = 1.0 + 0.1 * a
        out[k] = torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).to(torch.float32)
    return out


def all_weights(dseed, mlp_dim, pseed):
    w = R.draw_weights(dseed, mlp_dim)
    w.update(draw_prompt_weights(pseed))
    return w


def pack_mask_weights(w):
    """vdr_op_mask_embed's `weights`: the ten tensors back to back, fp32 [4684]"""
    return torch.cat([w[MD + k].reshape(-1).float() for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias",
                                                               "6.weight", "6.bias")])


# ---- the sparse rows ------------------------------------------------------------------------------------------------------
def sparse_tokens(w, img, boxes=None, points=None, labels=None):
    """-> [P, np + (2 if boxes else 1), 256] float64"""
    gauss = w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"]
    rows = []
    if points is not None:
        P = points.shape[0] * points.shape[1]
        pts, lb = points.double().reshape(P, -1, 2), labels.reshape(P, -1).long()
        if boxes is None:  # the padding point: a label -1 row
            pts = torch.cat([pts, torch.zeros((P, 1, 2), dtype=torch.float64)], dim=1)
            lb = torch.cat([lb, torch.full((P, 1), -1, dtype=torch.long)], dim=1)
        pe = R.fourier_pe((pts + 0.5) / float(img), gauss)
        nap = w["prompt_encoder.not_a_point_embed.weight"][0].double()
        row = torch.where((lb == -1)[..., None], nap.expand_as(pe), pe)
        row = torch.where((lb == -10)[..., None], torch.zeros_like(pe), row)
        for v in (0, 1):
            row = torch.where((lb == v)[..., None], row + w[f"prompt_encoder.point_embeddings.{v}.weight"][0].double(), row)
        rows.append(row)
    if boxes is not None:
        rows.append(R.box_tokens(boxes, img, w))
    elif points is None:
        raise ValueError("no prompt")
    return torch.cat(rows, dim=1)


# ---- the mask chain ---------------------------------------------------------------------------------------------------------
def _ln2d(x, g, b, eps):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double()[None, :, None, None] + b.double()[None, :, None, None]


def mask_dense(w, mask, eps):
    """mask [Pm, 4g, 4g] -> dense [Pm, 256, g, g] float64 (exact erf GELU)"""
    F = torch.nn.functional
    x = F.conv2d(mask.double()[:, None], w[MD + "0.weight"].double(), w[MD + "0.bias"].double(), stride=2)
    x = R.gelu(_ln2d(x, w[MD + "1.weight"], w[MD + "1.bias"], eps))
    x = F.conv2d(x, w[MD + "3.weight"].double(), w[MD + "3.bias"].double(), stride=2)
    x = R.gelu(_ln2d(x, w[MD + "4.weight"], w[MD + "4.bias"], eps))
    return F.conv2d(x, w[MD + "6.weight"].double(), w[MD + "6.bias"].double())


def _ln_err(c, e, g, b, eps, dim):
    """LayerNorm over `dim` of c carrying the entry-wise error e, as the device computes it (sequential sum, two-pass, IEEE sqrt
    and division) -> (y, ey), first order in e and u:
      d_i = c_i - mean:        |dd_i| <= e_i + mean(e) + (D + 1) u mean|c| + u |d_i|
      var = mean(d^2):         |dvar| <= mean(2 |d| dd) + (D + 2) u var
      r = (var + eps)^-1/2:    |dr| / r <= dvar / (2 (var + eps)) + 3 u
      y = (d r) g + b:         |dy| <= |g| r (dd + |d| dr / r) + 3 u |y - b| + u |y|"""
    D = c.shape[dim]
    mu = c.mean(dim, keepdim=True)
    d = c - mu
    dd = e + e.mean(dim, keepdim=True) + (D + 1) * U32 * c.abs().mean(dim, keepdim=True) + U32 * d.abs()
    var = (d * d).mean(dim, keepdim=True)
    dvar = (2 * d.abs() * dd).mean(dim, keepdim=True) + (D + 2) * U32 * var
    r = 1.0 / torch.sqrt(var + eps)
    drel = dvar / (2 * (var + eps)) + 3 * U32
    y = d * r * g + b
    ey = g.abs() * r * (dd + d.abs() * drel) + 3 * U32 * (y - b).abs() + U32 * y.abs()
    return y, ey


def _gelu_err(y, ey):
    a = R.gelu(y)
    return a, 1.13 * ey + R.GELU_ABS_ERR + 4 * U32 * a.abs()   # |gelu'| <= 1.13; the device polynomial's absolute error


def mask_embed_ref(emb, mask, w, eps, nb=1):
    """vdr_op_mask_embed in float64: emb [B, 256, g, g], mask [B * nb, 4g, 4g] or [B, 4g, 4g] -> (exact [P * n, 256] before the
    rounding to bf16, bound).  The bound follows the chain of include/vdr.h step by step: an fma chain of K terms from the bias
    errs by at most (K + 1) u (sum |w x| + |b|) plus |w| times the errors of its inputs; the LayerNorms by _ln_err; the GELUs by
    _gelu_err; the last addition by u |out|.  All first order; the total is doubled for the second-order terms."""
    B, C, g, _ = emb.shape
    P = B * nb
    m = mask.double()
    if m.shape[0] != P:
        m = m.repeat_interleave(nb, dim=0)
    x = m.reshape(P, g, 2, 2, g, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(P, g, g, 4, 4)   # [P, cy, cx, by*2+bx, dy*2+dx]
    W1, b1 = w[MD + "0.weight"].double().reshape(4, 4), w[MD + "0.bias"].double()
    c1 = torch.einsum("pyxsk,ck->pyxsc", x, W1) + b1                                           # [P, cy, cx, sub, ch]
    e1 = 5 * U32 * (torch.einsum("pyxsk,ck->pyxsc", x.abs(), W1.abs()) + b1.abs())
    y1, ey1 = _ln_err(c1, e1, w[MD + "1.weight"].double(), w[MD + "1.bias"].double(), eps, -1)
    a1, ea1 = _gelu_err(y1, ey1)
    W2, b2 = w[MD + "3.weight"].double().reshape(16, 4, 4), w[MD + "3.bias"].double()          # [co, ci, sub]
    c2 = torch.einsum("pyxsc,ocs->pyxo", a1, W2) + b2
    e2 = torch.einsum("pyxsc,ocs->pyxo", ea1, W2.abs()) + 17 * U32 * (torch.einsum("pyxsc,ocs->pyxo", a1.abs(), W2.abs()) + b2.abs())
    y2, ey2 = _ln_err(c2, e2, w[MD + "4.weight"].double(), w[MD + "4.bias"].double(), eps, -1)
    a2, ea2 = _gelu_err(y2, ey2)
    W3, b3 = w[MD + "6.weight"].double().reshape(C, 16), w[MD + "6.bias"].double()
    dense = torch.einsum("pyxk,ck->pyxc", a2, W3) + b3
    e3 = torch.einsum("pyxk,ck->pyxc", ea2, W3.abs()) + 17 * U32 * (torch.einsum("pyxk,ck->pyxc", a2.abs(), W3.abs()) + b3.abs())
    e = emb.double().permute(0, 2, 3, 1).repeat_interleave(nb, dim=0)                          # [P, cy, cx, c]
    out = dense + e
    bound = 2.0 * (e3 + U32 * out.abs())
    return out.reshape(P * g * g, C), bound.reshape(P * g * g, C)


# ---- the decode at any T ------------------------------------------------------------------------------------------------------
def decode(w, emb, cfg, boxes=None, points=None, labels=None, mask_input=None, mode="f64"):
    """-> (low_res_logits [B, nb, 4, 4g, 4g], iou [B, nb, 4]) float64.  mask_input [B * nb, 4g, 4g] or [B, 4g, 4g] (per image).
    sam_decoder_ref.decode run per problem (B' = P, nb' = 1) with the sparse rows exchanged for `sparse_tokens` and, with a mask
    prompt, the keys' additive term no_mask_embed exchanged for dense (emb + dense - no_mask is handed in: the float64 sum
    (emb + dense - no_mask) + no_mask differs from emb + dense by 1e-16 relative, nothing beside the bf16 rounding after it)."""
    lead = boxes if boxes is not None else points
    B, nb = lead.shape[0], lead.shape[1]
    P, g = B * nb, cfg.g
    sparse = sparse_tokens(w, cfg.img, boxes, points, labels)
    e = emb.double().repeat_interleave(nb, dim=0)
    if mask_input is not None:
        m = mask_input.reshape(-1, 4 * g, 4 * g)
        if m.shape[0] != P:
            m = m.repeat_interleave(nb, dim=0)
        e = e + mask_dense(w, m, cfg.ln2d_eps) - w["prompt_encoder.no_mask_embed.weight"].double().reshape(1, -1, 1, 1)
    saved = R.box_tokens
    R.box_tokens = lambda *_: sparse
    try:
        lg, iou = R.decode(w, e, torch.zeros((P, 1, 4)), cfg, mode)
    finally:
        R.box_tokens = saved
    return lg.reshape(B, nb, 4, 4 * g, 4 * g), iou.reshape(B, nb, 4)


# ---- mask_box -------------------------------------------------------------------------------------------------------------------
def mask_box_ref(logits, prev, img, margin=0.0, threshold=0.0):
    """vdr_op_mask_box in torch fp32, operation by operation: logits [P, H, W], prev [P, 4] -> (boxes [P, 4] fp32, area [P] int32)"""
    P, H, W = logits.shape
    on = logits > threshold
    area = on.reshape(P, -1).sum(1).to(torch.int32)
    xs, ys = on.any(dim=1), on.any(dim=2)                                                      # [P, W], [P, H]
    ix, iy = torch.arange(W, device=logits.device), torch.arange(H, device=logits.device)
    big = 1 << 30
    x0 = torch.where(xs, ix, big).amin(1).float()
    x1 = (torch.where(xs, ix, -1).amax(1) + 1).float()
    y0 = torch.where(ys, iy, big).amin(1).float()
    y1 = (torch.where(ys, iy, -1).amax(1) + 1).float()
    f = torch.tensor(float(img), dtype=torch.float32, device=logits.device)
    sx, sy = f / torch.tensor(float(W), dtype=torch.float32, device=logits.device), f / torch.tensor(float(H), dtype=torch.float32, device=logits.device)
    mg = torch.tensor(float(margin), dtype=torch.float32, device=logits.device)
    box = torch.stack([x0 * sx - mg, y0 * sy - mg, x1 * sx + mg, y1 * sy + mg], dim=1).clamp(0.0, float(img))
    return torch.where((area > 0)[:, None], box, prev.float()), area


# ---- the goldens ------------------------------------------------------------------------------------------------------------------
def golden_prompts(golden_dir, tag):
    """tests/golden/sam_hf_prompts_<tag>.npz -> (base case of sam_decoder_ref.golden_case with the prompt weights added, list of
    prompt sets: dict(name, boxes / points / labels / mask_input (tensors or None), all4, iou4, f64_diff, bf16_diff))"""
    base = R.golden_case(golden_dir, tag)
    z = np.load(os.path.join(golden_dir, f"sam_hf_prompts_{tag}.npz"), allow_pickle=False)
    base["weights"] = dict(base["weights"])
    base["weights"].update(draw_prompt_weights(int(z["pseed"])))
    assert R.weights_sha256(draw_prompt_weights(int(z["pseed"]))) == str(z["prompt_sha256"]), "the prompt weight recipe no longer draws the golden's bytes"
    sets = []
    for name in str(z["names"]).split(","):
        s = {"name": name}
        for k in ("boxes", "points", "labels", "mask_input"):
            s[k] = torch.from_numpy(z[f"{name}.{k}"]) if f"{name}.{k}" in z.files else None
        s["all4"], s["iou4"] = torch.from_numpy(z[f"{name}.all4"]).double(), torch.from_numpy(z[f"{name}.iou4"]).double()
        s["f64_diff"], s["bf16_diff"] = tuple(float(v) for v in z[f"{name}.f64_diff"]), tuple(float(v) for v in z[f"{name}.bf16_diff"])
        sets.append(s)
    return base, sets
