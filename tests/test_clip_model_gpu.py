"""GPU: CLIP / SigLIP vision towers end to end through the C ABI -- the committed transformers vectors of the tiny
models (tests/golden/clip_hf_tiny.npz, siglip_hf_tiny.npz), the full-size base models on seeded weights against the
fp32 restatement (tests/clip_ref.py), and the other outputs (other input sizes, intermediate layers, attention maps).

Gates: those of tests/test_model_gpu.py (per-row cosine >= 0.999, rel L2 <= gate(L) = 4e-3 + 3e-3 sqrt(L) against fp32
arithmetic and against the restatement with bf16 rounding emulated at the device's store points) and of
tests/test_fullsize_gpu.py (the same gate at full depth, plus duplicate rows / batch permutation / batch independence).
Outputs behind a head carry its roundings too: SigLIP's pooling head (k/v GEMM, attention, out-projection, LayerNorm,
MLP: a block's worth of bf16 stores) is gated as one more block, gate(L + 1); CLIP's image_embeds (one more bf16 GEMM
output) at gate(L) + 2e-3, as test_fullsize_gpu.py adds 2e-3 for a bf16 output rounding.
"""
import math
import os

import numpy as np
import pytest
import torch

import clip_ref as cr
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _min_cos(a, b):
    a, b = a.double().reshape(-1, a.shape[-1]), b.double().reshape(-1, b.shape[-1])
    return torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()


def gate_l2(layers):  # tests/test_model_gpu.py
    return 4e-3 + 3e-3 * math.sqrt(max(layers, 1))


def _gate(got, ref, ref_emul, l2_fp32, l2_emul, what):  # tests/test_model_gpu.py
    got = got.float().cpu()
    assert torch.isfinite(got).all(), what
    r32, re, c = _rel_l2(got, ref), _rel_l2(got, ref_emul), _min_cos(got, ref)
    print(f"{what}: relL2 vs fp32 {r32:.3e}  vs bf16-emulated {re:.3e}  min cos {c:.6f}")
    assert c >= 0.999, f"{what}: min cosine {c}"
    assert r32 <= l2_fp32, f"{what}: rel L2 vs fp32 {r32}"
    assert re <= l2_emul, f"{what}: rel L2 vs bf16-emulating restatement {re}"


def _check(got, ref, gate, min_cos, what):  # tests/test_fullsize_gpu.py
    got = got.float().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    r, c = _rel_l2(got, ref), _min_cos(got, ref)
    print(f"{what}: relL2 vs fp32 restatement {r:.3e} (gate {gate:.3e})  min row cosine {c:.6f} (gate {min_cos})")
    assert c >= min_cos, f"{what}: min cosine {c}"
    assert r <= gate, f"{what}: rel L2 {r} > {gate}"


def _vdr_cfg(c: vo.VitCfg, **kw):
    import vdr
    return vdr.VdrConfig(img=c.img, patch=c.patch, in_chans=3, dim=c.dim, heads=c.heads, layers=c.layers, mlp_hidden=c.mlp_hidden,
                         act=c.act, has_cls=c.has_cls, input_ln=c.input_ln, ln_eps=c.ln_eps, **kw)


def _tiny(golden_dir, family, **kw):
    """(golden, VitCfg, translated weights, model) of a tiny golden, loaded through load_model's key detection"""
    import vdr
    g = np.load(os.path.join(golden_dir, family + "_hf_tiny.npz"), allow_pickle=False)
    cfg = cr.tiny_cfg(g, family)
    sd = cr.golden_state_dict(g)
    name = f"_{family}_tiny_test"
    vdr.ARCHS[name] = _vdr_cfg(cfg)
    try:
        model = vdr.load_model(name, weights=sd, **kw)  # transformers keys: translated on the way in
    finally:
        del vdr.ARCHS[name]
    from vdr import weights as W
    w = (W.from_clip_vision_state_dict if family == "clip" else W.from_siglip_vision_state_dict)(sd)
    return g, cfg, w, model


def _tokens_raw(model, x):
    """the residual stream after the last block, no final norm (CLIP's last_hidden_state)"""
    import vdr
    return model.engine.forward_layers(x, [vdr.LayerOut(model.cfg.layers - 1, vdr.OUT_TOKENS, torch.float32, norm=False)])[0]


# ---- tiny goldens ---------------------------------------------------------------------------------------------------------
def test_clip_tiny_against_the_transformers_vectors(golden_dir):
    import vdr
    g, cfg, w, m = _tiny(golden_dir, "clip")
    L = cfg.layers
    x = torch.from_numpy(g["x"])
    emu = cr.clip_forward(cfg, w, x, emulate=True)
    xd = x.cuda()
    _gate(_tokens_raw(m, xd), torch.from_numpy(g["last_hidden_state"]), emu["last_hidden_state"], gate_l2(L), gate_l2(L), "clip last_hidden_state")
    pooled = m(xd)  # model(x) on a CLIP model: post-LayerNorm CLS, transformers' pooler_output
    assert pooled.shape == (x.shape[0], cfg.dim) and torch.equal(pooled, m.forward_features(xd))
    _gate(pooled, torch.from_numpy(g["pooler_output"]), emu["pooler_output"], gate_l2(L), gate_l2(L), "clip pooler_output")
    emb = m.get_image_features(xd)
    assert emb.shape == (x.shape[0], int(g["proj"])) and emb.dtype == torch.float32
    _gate(emb, torch.from_numpy(g["image_embeds"]), emu["image_embeds"], gate_l2(L) + 2e-3, gate_l2(L) + 2e-3, "clip image_embeds")
    nrm = m.get_image_features(xd, normalize=True)
    assert torch.allclose(nrm.norm(dim=-1), torch.ones(x.shape[0], device="cuda"), atol=1e-5)
    assert torch.allclose(nrm, emb / emb.norm(dim=-1, keepdim=True), atol=1e-6)
    # 64 x 32 (H x W) through set_input_size: transformers' interpolate_pos_encoding=True
    x2 = torch.from_numpy(g["x_64x32"])
    emu2 = cr.clip_forward(cfg, w, x2, emulate=True)
    m.set_input_size(64, 32)
    _gate(_tokens_raw(m, x2.cuda()), torch.from_numpy(g["last_hidden_state_64x32"]), emu2["last_hidden_state"], gate_l2(L), gate_l2(L),
          "clip last_hidden_state 64x32")
    _gate(m.get_image_features(x2.cuda()), torch.from_numpy(g["image_embeds_64x32"]), emu2["image_embeds"], gate_l2(L) + 2e-3,
          gate_l2(L) + 2e-3, "clip image_embeds 64x32")
    m.set_input_size(cfg.img, cfg.img)
    assert torch.equal(m.get_image_features(xd), emb), "back at the native size: the same bits"


def test_siglip_tiny_against_the_transformers_vectors(golden_dir):
    import vdr
    g, cfg, w, m = _tiny(golden_dir, "siglip")
    L = cfg.layers
    x = torch.from_numpy(g["x"])
    emu = cr.siglip_forward(cfg, w, x, emulate=True)
    xd = x.cuda()
    tok = m.engine.forward(xd, vdr.OUT_TOKENS)
    assert tok.shape == (x.shape[0], cfg.n_patches, cfg.dim)  # no CLS token
    _gate(tok, torch.from_numpy(g["last_hidden_state"]), emu["last_hidden_state"], gate_l2(L), gate_l2(L), "siglip last_hidden_state")
    pooled = m.get_image_features(xd)
    assert pooled.shape == (x.shape[0], cfg.dim) and pooled.dtype == torch.float32
    assert torch.equal(m(xd), pooled)  # model(x) on a SigLIP model: the pooled feature
    _gate(pooled, torch.from_numpy(g["pooler_output"]), emu["pooler_output"], gate_l2(L + 1), gate_l2(L + 1), "siglip pooler_output")
    with pytest.raises(Exception):
        m.forward_features(xd)  # no CLS token
    x2 = torch.from_numpy(g["x_64x32"])
    emu2 = cr.siglip_forward(cfg, w, x2, emulate=True)
    m.set_input_size(64, 32)
    _gate(m.engine.forward(x2.cuda(), vdr.OUT_TOKENS), torch.from_numpy(g["last_hidden_state_64x32"]), emu2["last_hidden_state"],
          gate_l2(L), gate_l2(L), "siglip last_hidden_state 64x32")
    _gate(m.get_image_features(x2.cuda()), torch.from_numpy(g["pooler_output_64x32"]), emu2["pooler_output"], gate_l2(L + 1),
          gate_l2(L + 1), "siglip pooler_output 64x32")


def test_clip_input_layernorm_keeps_the_fold_and_matches_the_explicit_path(golden_dir):
    """input_ln = 1 on an image model keeps the LayerNorm fold (the input LayerNorm leaves block 0's row statistics);
    no_ln_fold = 1 keeps the explicit path.  The assertions of test_model_gpu.py's fold on / off test."""
    import vdr
    g, cfg, w, fused_m = _tiny(golden_dir, "clip")
    _, _, _, plain_m = _tiny(golden_dir, "clip", ln_fold=False)
    x = torch.rand(16, 3, cfg.img, cfg.img, generator=torch.Generator().manual_seed(5))
    ref = cr.clip_forward(cfg, w, x)["tokens"]
    fused = fused_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    plain = plain_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    assert not torch.equal(fused, plain)  # two different code paths really ran
    gt = 1.5 * gate_l2(cfg.layers)
    r_f, r_p = _rel_l2(fused.cpu(), ref), _rel_l2(plain.cpu(), ref)
    print(f"CLIP tiny LN fold: fused {r_f:.3e}  explicit {r_p:.3e}  fused-vs-explicit {_rel_l2(fused.cpu(), plain.cpu()):.3e}")
    assert r_f <= gt and r_p <= gt
    assert r_f <= 1.25 * r_p, "folding LayerNorm must not cost accuracy"
    assert _rel_l2(fused.cpu(), plain.cpu()) <= gt
    assert _min_cos(fused.cpu(), ref) >= 0.999
    # the fold is really on: the profiler sees no LayerNorm launch per block, only the input LayerNorm (+ finalisers)
    for mdl, per_block in ((fused_m, False), (plain_m, True)):
        mdl.engine.profile(True)
        mdl.engine.forward(x.cuda(), vdr.OUT_TOKENS)
        torch.cuda.synchronize()
        prof = mdl.engine.profile_read()
        mdl.engine.profile(False)
        n_ln = prof.get("layernorm", {}).get("launches", 0)
        print("layernorm-class launches:", n_ln, "(fold on)" if not per_block else "(explicit)")
        # (explicit: the input LayerNorm + norm1 / norm2 of every block; fold on: the input LayerNorm alone -- a launch this
        # small finalises the row statistics inside the consuming GEMMs)
        assert n_ln == (1 + 2 * cfg.layers if per_block else 1)
    # layers and attention maps accept the combination too
    assert fused_m.get_intermediate_layers(x.cuda(), n=1)[0].shape == (16, cfg.n_patches, cfg.dim)


# ---- other outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_intermediate_layers_and_attention_maps_agree_with_the_restatement(golden_dir, family):
    g, cfg, w, m = _tiny(golden_dir, family)
    x = torch.rand(4, 3, cfg.img, cfg.img, generator=torch.Generator().manual_seed(9))
    ref = cr.tower(cfg, w, x, want_attn=True)
    ncls = 1 if cfg.has_cls else 0
    outs = m.get_intermediate_layers(x.cuda(), n=cfg.layers, norm=True, return_class_token=bool(ncls))
    raws = m.get_intermediate_layers(x.cuda(), n=cfg.layers, norm=False)
    for i in range(cfg.layers):
        normed = vo.layer_norm(ref["layers"][i], w["norm.weight"], w["norm.bias"], cfg.ln_eps)
        patch = outs[i][0] if ncls else outs[i]
        _check(patch, normed[:, ncls:], gate_l2(i + 1), 0.999, f"{family} block {i} patch tokens (norm)")
        if ncls:
            _check(outs[i][1], normed[:, 0], gate_l2(i + 1), 0.999, f"{family} block {i} cls (norm)")
        _check(raws[i], ref["layers"][i][:, ncls:], gate_l2(i + 1), 0.999, f"{family} block {i} patch tokens (raw)")
    # attention maps of every block on the folded path: the right block, head and row order against the restatement.  A
    # coarse check by design -- the scores come from bf16 q / k (2^-9 each) behind an activation that carries the forward's
    # rel-L2 (<= gate): |ds| of a few 1e-2 -> |dp| <= 0.1 p + 2e-3.  The softmax itself (scale, entry-wise error) is held
    # to derived bounds by test_attention_maps_match_a_float64_recompute_within_derived_bounds below.
    N = cfg.n_tokens
    maps = m.get_attention_maps(x.cuda(), layers=list(range(cfg.layers)), cls_only=False)
    for i, got in enumerate(maps):
        assert got.shape == (4, cfg.heads, N, N)
        want = ref["attn"][i]
        err = (got.cpu() - want).abs()
        assert (err <= 0.1 * want + 2e-3).all(), (family, i, err.max().item())
        assert torch.allclose(got.sum(-1).cpu(), torch.ones(4, cfg.heads, N), atol=1e-4)
    if ncls:
        row = m.get_attention_maps(x.cuda(), layers=cfg.layers - 1, cls_only=True)
        assert torch.equal(row, maps[-1][:, :, 0])


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_attention_maps_match_a_float64_recompute_within_derived_bounds(family):
    """The construction and the bounds of tests/test_attn_maps_gpu.py (test_maps_match_a_recompute_on_the_explicit_layernorm_path,
    which derives them) on a CLIP-shaped (QuickGELU, input LayerNorm, CLS) and a SigLIP-shaped (tanh-GELU, no CLS) tower:
    no_ln_fold, block l's input from the library's raw stream, norm1 by the library's LayerNorm op, qkv and the softmax in
    float64; |p - p64| <= p64 (2^(c (ds_k + max_j ds_j)) - 1) + p64 rel_fp32 + 1e-7, ds from the possible one-ulp flips of
    the stored bf16 q / k.  A softmax scale off by a percent moves peaked entries by several percent: far outside."""
    import vdr
    from vdr import ops
    from test_attn_maps_gpu import LOG2E, _block_input, _fp32_bounds, _softmax64
    clip = family == "clip"
    D, H = 64, 2
    dh = D // H
    cfg = vo.VitCfg(64, 16, 3, D, H, 3, 2 * D, act="quick_gelu" if clip else "gelu_tanh", has_cls=clip, input_ln=clip,
                    ln_eps=1e-5 if clip else 1e-6)
    w = vo.make_weights(cfg, seed=7 + dh, scale=0.05)
    for i in range(cfg.layers):  # (q / k rows scaled: scores of about 3 nats spread, attention far from uniform)
        w[f"blocks.{i}.attn.qkv.weight"][:2 * D] *= math.sqrt(1200.0 / D)
    e = vdr.Engine(_vdr_cfg(cfg, ln_fold=False))
    e.load_weights(w)
    N = cfg.n_tokens
    assert N == (17 if clip else 16)
    x = vo.make_images(cfg, 3, seed=9).cuda()
    B = x.shape[0]
    c = LOG2E / math.sqrt(dh)
    maps, bounds = {}, {}
    for layer in (1, 2):
        _, (got,) = e.forward_attn_maps(x, [vdr.AttnMap(layer, N)])
        xin = _block_input(e, x, layer).reshape(-1, D).to(torch.bfloat16).contiguous()
        h = ops.layernorm(xin, w[f"blocks.{layer}.norm1.weight"].cuda(), w[f"blocks.{layer}.norm1.bias"].cuda(), cfg.ln_eps,
                          torch.bfloat16).double()
        W = w[f"blocks.{layer}.attn.qkv.weight"].to(torch.bfloat16).double().cuda()
        bias = w[f"blocks.{layer}.attn.qkv.bias"].double().cuda()
        y = h @ W.T + bias
        err = (D + 2) * 2.0 ** -24 * (h.abs() @ W.abs().T + bias.abs())
        rn = y.to(torch.bfloat16)
        amb = ((y - err).to(torch.bfloat16) != rn) | ((y + err).to(torch.bfloat16) != rn)  # the stored value may be rn's neighbour
        mag = rn.double().abs().clamp_min(2.0 ** -126)
        ulp = torch.where(amb, torch.exp2(torch.floor(torch.log2(mag)) - 7), torch.zeros_like(y))  # bf16 spacing at rn
        qk, uq = rn.double().reshape(B, N, 3, H, dh), ulp.reshape(B, N, 3, H, dh)
        q, k = qk[:, :, 0].transpose(1, 2), qk[:, :, 1].transpose(1, 2)
        dq, dk = uq[:, :, 0].transpose(1, 2), uq[:, :, 1].transpose(1, 2)
        ds = dq @ k.abs().transpose(-1, -2) + q.abs() @ dk.transpose(-1, -2) + dq @ dk.transpose(-1, -2)
        ref = _softmax64(q, k, dh)
        rel_b, _ = _fp32_bounds(q.cpu(), k.cpu(), dh, N)
        bound = ref * (torch.exp2(c * (ds + ds.max(-1, keepdim=True).values)) - 1) + ref * rel_b + 1e-7
        got64 = got.double()
        worst = ((got64 - ref).abs() / bound).max().item()
        ent = -(ref * ref.clamp_min(1e-300).log()).sum(-1).mean().item()
        print(f"{family} block {layer}: max |dp| / bound {worst:.3f}  mean row entropy {ent:.3f} (log N {math.log(N):.3f})")
        assert torch.all((got64 - ref).abs() <= bound), worst
        assert ent < 0.8 * math.log(N), ent  # far from uniform
        maps[layer], bounds[layer] = got64, bound
    # the comparison tells heads and layers apart: their maps are at least 10x the bound apart, summed over the entries
    for layer in (1, 2):
        bd = bounds[layer]
        assert (maps[layer][:, 0] - maps[layer][:, 1]).abs().sum() >= 10 * (bd[:, 0] + bd[:, 1]).sum()
    assert (maps[1] - maps[2]).abs().sum() >= 10 * (bounds[1] + bounds[2]).sum()


# ---- full size ---------------------------------------------------------------------------------------------------------------
def _properties(run, x, small=3):
    """tests/test_fullsize_gpu.py: x [B, ...] on the device with x[B-1] == x[1]"""
    B = x.shape[0]
    out = run(x)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out[B - 1], out[1]), "duplicate images must give bitwise equal rows"
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B)).cuda()
    assert torch.equal(run(x[perm].contiguous()), out[perm]), "batch permutation equivariance"
    lo = B // 2
    assert torch.equal(run(x[lo:lo + small].contiguous()), out[lo:lo + small]), "a row depends on its batch"
    return out


@pytest.mark.parametrize("family,name", [("clip", "clip_vit_base16_224"), ("siglip", "siglip_base16_224")])
def test_base_models_all_twelve_blocks_batch_32(family, name):
    """Seeded random weights (SURVEY 8d's recipe), all 12 blocks, batch 32, every row against the fp32 restatement."""
    import vdr
    a = vdr.ARCHS[name]
    cfg = vo.VitCfg(a.img, a.patch, 3, a.dim, a.heads, a.layers, a.mlp_hidden, act=a.act, has_cls=a.has_cls, input_ln=a.input_ln,
                    ln_eps=a.ln_eps)
    assert cfg.layers == 12 and cfg.dim == 768
    w = cr.make_weights(cfg, family, seed=1)
    x = torch.rand(32, 3, cfg.img, cfg.img, generator=torch.Generator().manual_seed(3))
    x[31] = x[1]
    ref = (cr.clip_forward if family == "clip" else cr.siglip_forward)(cfg, w, x)
    m = vdr.load_model(name, weights=w)
    xd = x.cuda()
    ncls = 1 if cfg.has_cls else 0
    dense = _properties(lambda t: m.engine.forward(t, vdr.OUT_DENSE, torch.float32), xd)
    _check(dense, ref["tokens"][:, ncls:], gate_l2(12), 0.999, f"{name} L=12 dense")
    if family == "clip":
        cls = _properties(lambda t: m(t), xd)
        _check(cls, ref["pooler_output"], gate_l2(12), 0.999, f"{name} L=12 cls (pooler_output)")
        emb = _properties(lambda t: m.get_image_features(t), xd)
        assert emb.shape == (32, 512)
        _check(emb, ref["image_embeds"], gate_l2(12) + 2e-3, 0.999, f"{name} L=12 image_embeds")
    else:
        pooled = _properties(lambda t: m(t), xd)
        assert pooled.shape == (32, 768)
        _check(pooled, ref["pooler_output"], gate_l2(13), 0.999, f"{name} L=12 pooled (pooler_output)")
