"""GPU: DINOv3 and DINOv2-with-registers end to end through the C ABI -- the committed transformers vectors of the tiny
models (tests/golden/dinov3_hf_tiny.npz, dinov3_hf_gated_hd64.npz, dinov2reg_hf_tiny.npz) through load_model, the
prefix-row semantics of every output mode, and one full-size model of each family on seeded weights against the fp32
restatement (tests/dinov3_ref.py).

Gates: those of tests/model_gates.py as tests/test_clip_model_gpu.py applies them -- per-row cosine >= 0.999 and rel L2
<= gate(L) = 4e-3 + 3e-3 sqrt(L) against fp32 arithmetic and against the restatement with bf16 rounding emulated at the
device's store points (for DINOv3 that includes the bf16 qkv before the rotation and the bf16 q / k after it).
"""
import os

import numpy as np
import pytest
import torch

import dinov3_ref as dr
from model_gates import check_parity, gate_l2, min_cos, rel_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

GOLDENS = {"dinov3_hf_tiny": "dinov3", "dinov3_hf_gated_hd64": "dinov3", "dinov2reg_hf_tiny": "dinov2reg"}


def _tiny(golden_dir, name, **kw):
    """(golden, RegCfg, translated weights, model) of a tiny golden, loaded through load_model's key detection"""
    import vdr
    from vdr import weights as W
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    family = GOLDENS[name]
    rc = dr.golden_cfg(g, family)
    sd = dr.golden_state_dict(g)
    arch = f"_{name}_test"
    vdr.ARCHS[arch] = dr.vdr_config(rc)
    try:
        model = vdr.load_model(arch, weights=sd, **kw)  # transformers keys: translated on the way in
    finally:
        del vdr.ARCHS[arch]
    w = (W.from_dinov3_vit_state_dict if family == "dinov3" else W.from_dinov2_hf_state_dict)(sd)
    return g, rc, w, model


# ---- tiny goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_tiny_models_against_the_transformers_vectors(golden_dir, name):
    import vdr
    g, rc, w, m = _tiny(golden_dir, name)
    L, P, D = rc.vit.layers, rc.n_prefix, rc.vit.dim

    def run(tag):
        x = torch.from_numpy(g["x" + tag])
        emu = dr.forward(rc, w, x, emulate=True)
        hf = torch.from_numpy(g["last_hidden_state" + tag])
        xd = x.cuda()
        tok = m.engine.forward(xd, vdr.OUT_TOKENS)
        n = m.engine.n_patches
        assert tok.shape == (x.shape[0], P + n, D) and m.engine.n_tokens == P + n
        check_parity(tok, hf, f"{name}{tag} tokens (last_hidden_state)", gate_l2(L), emu["tokens"])
        cls = m(xd)
        check_parity(cls, torch.from_numpy(g["pooler_output" + tag]), f"{name}{tag} cls (pooler_output)", gate_l2(L),
                     emu["cls"])
        dense = m.engine.forward(xd, vdr.OUT_DENSE)
        assert dense.shape == (x.shape[0], n, D)
        check_parity(dense, hf[:, P:], f"{name}{tag} dense (patch rows)", gate_l2(L), emu["dense"])
        return tok

    native = run("")
    if "x_64x32" in g.files:  # DINOv3: no table, the RoPE angles follow the grid -- transformers at every size
        m.set_input_size(64, 32)
        assert m.grid == (8, 4)
        run("_64x32")
    else:  # another size runs (the DINOv2 golden: against the restatement's non-antialiased resampling)
        m.set_input_size(2 * rc.vit.img, rc.vit.img)
        x2 = torch.rand(2, 3, 2 * rc.vit.img, rc.vit.img, generator=torch.Generator().manual_seed(4))
        tok2 = m.engine.forward(x2.cuda(), vdr.OUT_TOKENS)
        check_parity(tok2, dr.forward(rc, w, x2)["tokens"], f"{name} 2:1 tokens", gate_l2(L),
                     dr.forward(rc, w, x2, emulate=True)["tokens"])
    m.set_input_size(rc.vit.img, rc.vit.img)
    assert torch.equal(m.engine.forward(torch.from_numpy(g["x"]).cuda(), vdr.OUT_TOKENS), native), "back at the native size: the same bits"


def test_dynamic_size_follows_the_images(golden_dir):
    import vdr
    g, rc, w, m = _tiny(golden_dir, "dinov3_hf_tiny", dynamic_size=True)
    x2 = torch.from_numpy(g["x_64x32"])
    emu = dr.forward(rc, w, x2, emulate=True)
    check_parity(m(x2.cuda()), torch.from_numpy(g["pooler_output_64x32"]), "dynamic_size 64x32 cls", gate_l2(rc.vit.layers),
                 emu["cls"])
    assert m.input_size == (64, 32)
    d = vdr.extract_dense(m, torch.from_numpy(g["x"]).cuda())
    assert d.shape == (3, 4, 4, rc.vit.dim) and m.input_size == (32, 32)
    check_parity(torch.from_numpy(d).reshape(3, 16, -1), torch.from_numpy(g["last_hidden_state"])[:, rc.n_prefix:],
                 "extract_dense", gate_l2(rc.vit.layers), dr.forward(rc, w, torch.from_numpy(g["x"]), emulate=True)["dense"])


# ---- prefix rows in every output mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dinov3_hf_tiny", "dinov2reg_hf_tiny"])
def test_output_modes_take_the_patch_rows_behind_the_prefix(golden_dir, name):
    import vdr
    g, rc, w, m = _tiny(golden_dir, name)
    L, P, D = rc.vit.layers, rc.n_prefix, rc.vit.dim
    assert P == 5
    x = torch.from_numpy(g["x"]).cuda()
    B, n = x.shape[0], m.engine.n_patches
    tok = m.engine.forward(x, vdr.OUT_TOKENS)
    assert torch.equal(m.engine.forward(x, vdr.OUT_DENSE), tok[:, P:]), "DENSE is rows P.. of TOKENS"
    assert torch.equal(m.engine.forward(x, vdr.OUT_CLS), tok[:, 0]) and torch.equal(m(x), tok[:, 0]), "CLS is row 0"
    (patch, cls), = m.get_intermediate_layers(x, n=1, return_class_token=True)
    assert torch.equal(patch, tok[:, P:]) and torch.equal(cls, tok[:, 0])
    (grid_map,) = m.get_intermediate_layers(x, n=1, reshape=True)
    gh, gw = m.grid
    assert torch.equal(grid_map, tok[:, P:].reshape(B, gh, gw, D).permute(0, 3, 1, 2))
    raw_tok, raw_dense, pooled, pooled_raw = m.engine.forward_layers(x, [
        vdr.LayerOut(L - 1, vdr.OUT_TOKENS, norm=False), vdr.LayerOut(L - 1, vdr.OUT_DENSE, norm=False),
        vdr.LayerOut(L - 1, vdr.OUT_POOLED), vdr.LayerOut(L - 1, vdr.OUT_POOLED, norm=False)])
    assert torch.equal(raw_dense, raw_tok[:, P:])
    # POOLED: the fp32 mean over rows P.. (n = 16 or 4 rows: one chunk summed in row order, times RN(1 / n)).  Each of the n
    # adds rounds a partial sum <= n max|row| (2^-24 relative), then the product: |error| <= (n + 2) 2^-24 max|row|
    for got, rows in ((pooled, tok), (pooled_raw, raw_tok)):
        want = rows[:, P:].double().mean(1)
        with_registers = rows[:, 1:].double().mean(1)
        err = (got.double() - want).abs().max().item()
        assert err <= (n + 2) * 2.0 ** -24 * rows[:, P:].abs().max().item(), err
        assert (got.double() - with_registers).abs().max().item() > 1e-3, "the register rows are not averaged in"
    feats = m.linear_probe_features(x, n_last_blocks=2)
    assert feats.shape == (B, 3 * D) and torch.equal(feats[:, D:2 * D], tok[:, 0]) and torch.equal(feats[:, 2 * D:], pooled)
    assert torch.equal(torch.from_numpy(vdr.extract_dense(m, x)).cuda(), tok[:, P:].reshape(B, gh, gw, D))
    # attention maps keep all N key columns; q_rows = 1 is the CLS row; reshape drops the P prefix columns
    N = P + n
    full = m.get_attention_maps(x, cls_only=False)
    assert full.shape == (B, rc.vit.heads, N, N) and torch.equal(m.get_last_selfattention(x), full)
    assert torch.allclose(full.sum(-1).cpu(), torch.ones(B, rc.vit.heads, N), atol=1e-4)
    row = m.get_attention_maps(x, cls_only=True)
    assert row.shape == (B, rc.vit.heads, N) and torch.equal(row, full[:, :, 0])
    shaped = m.get_attention_maps(x, cls_only=True, reshape=True)
    assert shaped.shape == (B, rc.vit.heads, gh, gw) and torch.equal(shaped, full[:, :, 0, P:].reshape(B, rc.vit.heads, gh, gw))
    mean = m.get_attention_maps(x, cls_only=True, head_mean=True, reshape=True)
    assert mean.shape == (B, gh, gw)


@pytest.mark.parametrize("name", ["dinov3_hf_tiny", "dinov2reg_hf_tiny"])
def test_layers_and_attention_maps_agree_with_the_restatement(golden_dir, name):
    g, rc, w, m = _tiny(golden_dir, name)
    c, P = rc.vit, rc.n_prefix
    x = torch.rand(4, 3, c.img, c.img, generator=torch.Generator().manual_seed(9))
    ref = dr.forward(rc, w, x, want_attn=True)
    emu = dr.forward(rc, w, x, emulate=True)
    outs = m.get_intermediate_layers(x.cuda(), n=c.layers, norm=True, return_class_token=True)
    raws = m.get_intermediate_layers(x.cuda(), n=c.layers, norm=False)
    for i in range(c.layers):
        normed = vo.layer_norm(ref["layers"][i], w["norm.weight"], w["norm.bias"], c.ln_eps)
        normed_e = vo.layer_norm(emu["layers"][i], w["norm.weight"], w["norm.bias"], c.ln_eps)
        check_parity(outs[i][0], normed[:, P:], f"{name} block {i} patch tokens (norm)", gate_l2(i + 1), normed_e[:, P:])
        check_parity(outs[i][1], normed[:, 0], f"{name} block {i} cls (norm)", gate_l2(i + 1), normed_e[:, 0])
        check_parity(raws[i], ref["layers"][i][:, P:], f"{name} block {i} patch tokens (raw)", gate_l2(i + 1),
                     emu["layers"][i][:, P:])
    # the maps come from the ROTATED q / k (DINOv3): the coarse check of tests/test_clip_model_gpu.py -- bf16 q / k behind
    # an activation that carries the forward's rel-L2: |dp| <= 0.1 p + 2e-3
    N = m.engine.n_tokens
    maps = m.get_attention_maps(x.cuda(), layers=list(range(c.layers)), cls_only=False)
    for i, got in enumerate(maps):
        want = ref["attn"][i]
        assert got.shape == want.shape == (4, c.heads, N, N)
        err = (got.cpu() - want).abs()
        assert (err <= 0.1 * want + 2e-3).all(), (name, i, err.max().item())
        assert torch.allclose(got.sum(-1).cpu(), torch.ones(4, c.heads, N), atol=1e-4)
    if rc.rope:  # the rotation matters to the maps: without it they are far outside the same band
        import dataclasses
        flat = dr.forward(dataclasses.replace(rc, rope=False), w, x, want_attn=True)["attn"][0]
        assert not ((maps[0].cpu() - flat).abs() <= 0.1 * flat + 2e-3).all()


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_layernorm_fold_on_and_off(golden_dir, name):
    """The prefix rows leave their (sum, sumsq) partials for the fold; no_ln_fold = 1 keeps the explicit path.  The
    assertions of the CLIP fold on / off test."""
    import vdr
    g, rc, w, fused_m = _tiny(golden_dir, name)
    _, _, _, plain_m = _tiny(golden_dir, name, ln_fold=False)
    c = rc.vit
    x = torch.rand(16, 3, c.img, c.img, generator=torch.Generator().manual_seed(5))
    ref = dr.forward(rc, w, x)["tokens"]
    fused = fused_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    plain = plain_m.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    assert not torch.equal(fused, plain)  # two different code paths really ran
    gt = gate_l2(c.layers)
    r_f, r_p = rel_l2(fused.cpu(), ref), rel_l2(plain.cpu(), ref)
    print(f"{name} LN fold: fused {r_f:.3e}  explicit {r_p:.3e}  fused-vs-explicit {rel_l2(fused.cpu(), plain.cpu()):.3e}  (gate {gt:.3e})")
    assert r_f <= gt and r_p <= gt
    assert min_cos(fused.cpu(), ref) >= 0.999 and min_cos(plain.cpu(), ref) >= 0.999
    for mdl, per_block in ((fused_m, False), (plain_m, True)):
        mdl.engine.profile(True)
        mdl.engine.forward(x.cuda(), vdr.OUT_TOKENS)
        torch.cuda.synchronize()
        prof = mdl.engine.profile_read()
        mdl.engine.profile(False)
        assert prof.get("layernorm", {}).get("launches", 0) == (2 * c.layers if per_block else 0)
        # the prefix rows are one launch; with RoPE every block adds one rotation, booked in the same class
        assert prof["assemble"]["launches"] == 1 + (c.layers if rc.rope else 0)


# ---- full size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["dinov3_vitb16", "dinov2_small14_reg_518"])
def test_full_size_models_batch_8(arch):
    """Seeded random weights (SURVEY 8d's recipe), every block, batch 8, every row against the fp32 restatement."""
    import vdr
    a = vdr.ARCHS[arch]
    vit = vo.VitCfg(a.img, a.patch, 3, a.dim, a.heads, a.layers, a.mlp_hidden, act=a.act, layerscale=a.layerscale, has_pos=a.has_pos,
                    ln_eps=a.ln_eps)
    rc = dr.RegCfg(vit, a.n_register, a.rope, a.rope_theta)
    assert a.layers == 12 and rc.n_prefix == 5
    w = dr.make_weights(rc, seed=1)
    x = torch.rand(8, 3, a.img, a.img, generator=torch.Generator().manual_seed(3))
    x[7] = x[1]
    ref = dr.forward(rc, w, x)
    m = vdr.load_model(arch, weights=w)
    xd = x.cuda()
    tok = m.engine.forward(xd, vdr.OUT_TOKENS)
    assert tok.shape == (8, 5 + vit.n_patches, a.dim)
    assert torch.equal(tok[7], tok[1]), "duplicate images must give bitwise equal rows"
    for got, want, what in ((tok, ref["tokens"], "tokens"), (m(xd), ref["cls"], "cls"),
                            (m.engine.forward(xd, vdr.OUT_DENSE), ref["dense"], "dense")):
        check_parity(got, want, f"{arch} L=12 {what}", gate_l2(12))
    assert torch.equal(m.engine.forward(xd, vdr.OUT_DENSE), tok[:, 5:])
