"""GPU: CLIP / SigLIP vision towers end to end through the C ABI -- the committed transformers vectors of the tiny
models (tests/golden/clip_hf_tiny.npz, siglip_hf_tiny.npz), the full-size base models on seeded weights against the
fp32 restatement (tests/clip_ref.py), and the other outputs (other input sizes, intermediate layers, attention maps).

Gates: those of tests/model_gates.py (per-row cosine >= 0.999, rel L2 <= gate(L) = 4e-3 + 3e-3 sqrt(L) against fp32
arithmetic and against the restatement with bf16 rounding emulated at the device's store points) and of
tests/test_fullsize_gpu.py (the same gate at full depth, plus duplicate rows / batch permutation / batch independence).
Outputs behind a head carry its roundings too: SigLIP's pooling head (k/v GEMM, attention, out-projection, LayerNorm,
MLP: a block's worth of bf16 stores) is gated as one more block, gate(L + 1); CLIP's image_embeds (one more bf16 GEMM
output) at gate(L) + 2e-3, as test_fullsize_gpu.py adds 2e-3 for a bf16 output rounding.
"""
import math

import pytest
import torch

import clip_ref as cr
import handle_configs as hc
from attn_maps_ref import LOG2E, block_input, fp32_bounds, softmax64
from model_gates import check_batch_properties, check_parity, gate_l2, min_cos, rel_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


def _tokens_raw(model, x):
    """the residual stream after the last block, no final norm (CLIP's last_hidden_state)"""
    import vdr
    return model.engine.forward_layers(x, [vdr.LayerOut(model.cfg.layers - 1, vdr.OUT_TOKENS, torch.float32, norm=False)])[0]


# ---- tiny goldens ---------------------------------------------------------------------------------------------------------
def test_clip_tiny_against_the_transformers_vectors(golden_dir):
    import vdr
    g, cfg, w, m = cr.tiny_model(golden_dir, "clip")
    L = cfg.layers
    x = torch.from_numpy(g["x"])
    emu = cr.clip_forward(cfg, w, x, emulate=True)
    xd = x.cuda()
    check_parity(_tokens_raw(m, xd), torch.from_numpy(g["last_hidden_state"]), "clip last_hidden_state", gate_l2(L),
                 emu["last_hidden_state"])
    pooled = m(xd)  # model(x) on a CLIP model: post-LayerNorm CLS, transformers' pooler_output
    assert pooled.shape == (x.shape[0], cfg.dim) and torch.equal(pooled, m.forward_features(xd))
    check_parity(pooled, torch.from_numpy(g["pooler_output"]), "clip pooler_output", gate_l2(L), emu["pooler_output"])
    emb = m.get_image_features(xd)
    assert emb.shape == (x.shape[0], int(g["proj"])) and emb.dtype == torch.float32
    check_parity(emb, torch.from_numpy(g["image_embeds"]), "clip image_embeds", gate_l2(L) + 2e-3, emu["image_embeds"])
    nrm = m.get_image_features(xd, normalize=True)
    assert torch.allclose(nrm.norm(dim=-1), torch.ones(x.shape[0], device="cuda"), atol=1e-5)
    assert torch.allclose(nrm, emb / emb.norm(dim=-1, keepdim=True), atol=1e-6)
    # 64 x 32 (H x W) through set_input_size: transformers' interpolate_pos_encoding=True
    x2 = torch.from_numpy(g["x_64x32"])
    emu2 = cr.clip_forward(cfg, w, x2, emulate=True)
    m.set_input_size(64, 32)
    check_parity(_tokens_raw(m, x2.cuda()), torch.from_numpy(g["last_hidden_state_64x32"]), "clip last_hidden_state 64x32",
                 gate_l2(L), emu2["last_hidden_state"])
    check_parity(m.get_image_features(x2.cuda()), torch.from_numpy(g["image_embeds_64x32"]), "clip image_embeds 64x32",
                 gate_l2(L) + 2e-3, emu2["image_embeds"])
    m.set_input_size(cfg.img, cfg.img)
    assert torch.equal(m.get_image_features(xd), emb), "back at the native size: the same bits"


def test_siglip_tiny_against_the_transformers_vectors(golden_dir):
    import vdr
    g, cfg, w, m = cr.tiny_model(golden_dir, "siglip")
    L = cfg.layers
    x = torch.from_numpy(g["x"])
    emu = cr.siglip_forward(cfg, w, x, emulate=True)
    xd = x.cuda()
    tok = m.engine.forward(xd, vdr.OUT_TOKENS)
    assert tok.shape == (x.shape[0], cfg.n_patches, cfg.dim)  # no CLS token
    check_parity(tok, torch.from_numpy(g["last_hidden_state"]), "siglip last_hidden_state", gate_l2(L),
                 emu["last_hidden_state"])
    pooled = m.get_image_features(xd)
    assert pooled.shape == (x.shape[0], cfg.dim) and pooled.dtype == torch.float32
    assert torch.equal(m(xd), pooled)  # model(x) on a SigLIP model: the pooled feature
    check_parity(pooled, torch.from_numpy(g["pooler_output"]), "siglip pooler_output", gate_l2(L + 1), emu["pooler_output"])
    with pytest.raises(Exception):
        m.forward_features(xd)  # no CLS token
    x2 = torch.from_numpy(g["x_64x32"])
    emu2 = cr.siglip_forward(cfg, w, x2, emulate=True)
    m.set_input_size(64, 32)
    check_parity(m.engine.forward(x2.cuda(), vdr.OUT_TOKENS), torch.from_numpy(g["last_hidden_state_64x32"]),
                 "siglip last_hidden_state 64x32", gate_l2(L), emu2["last_hidden_state"])
    check_parity(m.get_image_features(x2.cuda()), torch.from_numpy(g["pooler_output_64x32"]), "siglip pooler_output 64x32",
                 gate_l2(L + 1), emu2["pooler_output"])


def test_clip_input_layernorm_keeps_the_fold_and_matches_the_explicit_path(golden_dir):
    """input_ln = 1 on an image model keeps the LayerNorm fold (the input LayerNorm leaves block 0's row statistics);
    no_ln_fold = 1 keeps the explicit path.  The assertions of test_model_gpu.py's fold on / off test."""
    import vdr
    g, cfg, w, fused_m = cr.tiny_model(golden_dir, "clip")
    _, _, _, plain_m = cr.tiny_model(golden_dir, "clip", ln_fold=False)
    x = torch.rand(16, 3, cfg.img, cfg.img, generator=torch.Generator().manual_seed(5))
    ref = cr.clip_forward(cfg, w, x)["tokens"]
    fused = fused_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    plain = plain_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    assert not torch.equal(fused, plain)  # two different code paths really ran
    gt = 1.5 * gate_l2(cfg.layers)
    r_f, r_p = rel_l2(fused.cpu(), ref), rel_l2(plain.cpu(), ref)
    print(f"CLIP tiny LN fold: fused {r_f:.3e}  explicit {r_p:.3e}  fused-vs-explicit {rel_l2(fused.cpu(), plain.cpu()):.3e}")
    assert r_f <= gt and r_p <= gt
    assert r_f <= 1.25 * r_p, "folding LayerNorm must not cost accuracy"
    assert rel_l2(fused.cpu(), plain.cpu()) <= gt
    assert min_cos(fused.cpu(), ref) >= 0.999
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
    g, cfg, w, m = cr.tiny_model(golden_dir, family)
    x = torch.rand(4, 3, cfg.img, cfg.img, generator=torch.Generator().manual_seed(9))
    ref = cr.tower(cfg, w, x, want_attn=True)
    ncls = 1 if cfg.has_cls else 0
    outs = m.get_intermediate_layers(x.cuda(), n=cfg.layers, norm=True, return_class_token=bool(ncls))
    raws = m.get_intermediate_layers(x.cuda(), n=cfg.layers, norm=False)
    for i in range(cfg.layers):
        normed = vo.layer_norm(ref["layers"][i], w["norm.weight"], w["norm.bias"], cfg.ln_eps)
        patch = outs[i][0] if ncls else outs[i]
        check_parity(patch, normed[:, ncls:], f"{family} block {i} patch tokens (norm)", gate_l2(i + 1))
        if ncls:
            check_parity(outs[i][1], normed[:, 0], f"{family} block {i} cls (norm)", gate_l2(i + 1))
        check_parity(raws[i], ref["layers"][i][:, ncls:], f"{family} block {i} patch tokens (raw)", gate_l2(i + 1))
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
    clip = family == "clip"
    D, H = 64, 2
    dh = D // H
    cfg = vo.VitCfg(64, 16, 3, D, H, 3, 2 * D, act="quick_gelu" if clip else "gelu_tanh", has_cls=clip, input_ln=clip,
                    ln_eps=1e-5 if clip else 1e-6)
    w = vo.make_weights(cfg, seed=7 + dh, scale=0.05)
    for i in range(cfg.layers):  # (q / k rows scaled: scores of about 3 nats spread, attention far from uniform)
        w[f"blocks.{i}.attn.qkv.weight"][:2 * D] *= math.sqrt(1200.0 / D)
    e = hc.engine(cfg, w, ln_fold=False)
    N = cfg.n_tokens
    assert N == (17 if clip else 16)
    x = vo.make_images(cfg, 3, seed=9).cuda()
    B = x.shape[0]
    c = LOG2E / math.sqrt(dh)
    maps, bounds = {}, {}
    for layer in (1, 2):
        _, (got,) = e.forward_attn_maps(x, [vdr.AttnMap(layer, N)])
        xin = block_input(e, x, layer).reshape(-1, D).to(torch.bfloat16).contiguous()
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
        ref = softmax64(q, k, dh)
        rel_b, _ = fp32_bounds(q.cpu(), k.cpu(), dh, N)
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
    dense = check_batch_properties(lambda t: m.engine.forward(t, vdr.OUT_DENSE, torch.float32), xd)
    check_parity(dense, ref["tokens"][:, ncls:], f"{name} L=12 dense", gate_l2(12))
    if family == "clip":
        cls = check_batch_properties(lambda t: m(t), xd)
        check_parity(cls, ref["pooler_output"], f"{name} L=12 cls (pooler_output)", gate_l2(12))
        emb = check_batch_properties(lambda t: m.get_image_features(t), xd)
        assert emb.shape == (32, 512)
        check_parity(emb, ref["image_embeds"], f"{name} L=12 image_embeds", gate_l2(12) + 2e-3)
    else:
        pooled = check_batch_properties(lambda t: m(t), xd)
        assert pooled.shape == (32, 768)
        check_parity(pooled, ref["pooler_output"], f"{name} L=12 pooled (pooler_output)", gate_l2(13))
