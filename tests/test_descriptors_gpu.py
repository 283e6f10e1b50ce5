"""GPU: facet descriptors inside the forward -- vdr_forward_facets / Engine.forward_descriptors /
VitDescriptorModel.extract_descriptors on tiny configurations.

Gates (test 1, 7, 8): those of tests/test_model_gpu.py as test_golden_transformers_crosscheck applies them to `tokens` --
per-row cosine >= 0.999, rel L2 <= gate_l2(i + 1) = 4e-3 + 3e-3 sqrt(i + 1) for block i, against fp32 (the transformers
golden / the fp32 restatement) and against the restatement with bf16 rounding emulated at the device's store points
(tests/descriptor_ref.py facets).  q / k / v pass the stream's gate unchanged.  Measured on an MI355X (vit_hf_facets, rel
L2 against the fp32 golden / against the emulating restatement; the emulating restatement itself is 3.6e-3 .. 4.5e-3 from
the golden): block 0 (gate 7.0e-3) query 3.1e-3 / 3.5e-3, key 3.4e-3 / 3.6e-3, value 3.5e-3 / 3.4e-3, token 3.7e-3 /
2.9e-3; block 1 (gate 8.2e-3) query 3.9e-3 / 4.4e-3, key 3.9e-3 / 4.4e-3, value 4.2e-3 / 4.4e-3, token 4.6e-3 / 4.1e-3;
DINOv3 tiny, pre-rotation keys: 3.5e-3 / 3.7e-3 (block 0), 4.6e-3 / 4.9e-3 (block 1); min row cosine 0.99997.
Everything else is bitwise: a facet is a copy of rows the forward computes anyway, and its log-bin is vdr_op_log_bin of
those rows."""
import os

import numpy as np
import pytest
import torch

import descriptor_ref as dref
import dinov3_ref as dr
import handle_configs as hc
from handle_configs import P16, TINY  # the vit_hf_tiny / vit_hf_facets network; test_model_gpu.SMALL["p16_d128"]
from model_gates import check_parity, gate_l2, rel_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

FACETS = ("query", "key", "value", "token")


def _tiny():
    w = vo.make_weights(TINY, seed=21, scale=0.05)
    return w, vo.make_images(TINY, 2, seed=6)


def _model(monkeypatch, cfg, w, name="_facet_tiny", **kw):
    import vdr
    monkeypatch.setitem(vdr.ARCHS, name, hc.vit_config(cfg))
    return vdr.load_model(name, weights=w, **kw)


# ---- 1. the transformers golden ------------------------------------------------------------------------------------------
def test_hf_golden_every_facet_of_both_layers(golden_dir):
    import vdr
    g = np.load(os.path.join(golden_dir, "vit_hf_facets.npz"), allow_pickle=False)
    w, x = _tiny()
    emu = dref.facets(dref.plain(TINY), w, x, emulate=True)
    e = hc.engine(TINY, w)
    req = [vdr.FacetOut(i, f, all_rows=True) for i in range(TINY.layers) for f in FACETS]
    got, _, _ = e.forward_descriptors(x.cuda(), req)
    for r, t in zip(req, got):
        gl = gate_l2(r.layer + 1)
        check_parity(t, torch.from_numpy(g[f"{r.facet}.{r.layer}"]), f"vit_hf_facets {r.facet}.{r.layer}", gl,
                     emu[r.facet][r.layer])


# ---- 2. token == forward_layers(norm=False) ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(resid_fp32=True), dict(ln_fold=False)], ids=["fold", "resid32", "nofold"])
def test_token_facet_is_the_raw_layer_output_bitwise(kw):
    import vdr
    w = vo.make_weights(P16, seed=3, scale=0.05)
    x = vo.make_images(P16, 3, seed=4).cuda()
    e = hc.engine(P16, w, **kw)
    for dt in (torch.float32, torch.bfloat16):
        for i in range(P16.layers):
            want = e.forward_layers(x, [vdr.LayerOut(i, vdr.OUT_DENSE, dt, False), vdr.LayerOut(i, vdr.OUT_TOKENS, dt, False)])
            got, _, _ = e.forward_descriptors(x, [vdr.FacetOut(i, "token", dtype=dt), vdr.FacetOut(i, "token", all_rows=True, dtype=dt)])
            assert got[0].shape == (3, P16.n_patches, P16.dim) and got[1].shape == (3, P16.n_tokens, P16.dim)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kw, dt, i)


# ---- 3. binned == ops.log_bin(unbinned bf16 facet) -----------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, (16, 32)], ids=["4x4", "2x4"])
def test_binned_facet_is_log_bin_of_the_unbinned_bf16_facet(size):
    import vdr
    from vdr import ops
    w, _ = _tiny()
    e = hc.engine(TINY, w)
    if size:
        e.set_input_size(*size)
    H, W = e.input_size
    gh, gw = e.grid
    assert (gh, gw) == ((4, 4) if size is None else (2, 4))
    x = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(9)).cuda()
    for f in ("key", "token"):
        for i in range(TINY.layers):
            (plain16, binned, binned16), _, _ = e.forward_descriptors(x, [vdr.FacetOut(i, f, dtype=torch.bfloat16), vdr.FacetOut(i, f, 2),
                                                                          vdr.FacetOut(i, f, 2, dtype=torch.bfloat16)])
            assert binned.shape == (3, gh * gw, 17 * TINY.dim)
            assert torch.equal(binned, ops.log_bin(plain16, gh, gw, 2, torch.float32)), (f, i)
            assert torch.equal(binned16, ops.log_bin(plain16, gh, gw, 2, torch.bfloat16)), (f, i)
            assert torch.equal(binned[:, :, 4 * TINY.dim:5 * TINY.dim], plain16.float())


# ---- 4. one call == the separate calls -----------------------------------------------------------------------------------
def test_one_call_with_outs_maps_and_facets_equals_the_separate_calls():
    import vdr
    w = vo.make_weights(P16, seed=3, scale=0.05)
    x = vo.make_images(P16, 4, seed=4).cuda()
    e = hc.engine(P16, w)
    N = P16.n_tokens
    outs = [vdr.LayerOut(2, vdr.OUT_CLS), vdr.LayerOut(0, vdr.OUT_DENSE, torch.bfloat16, False), vdr.LayerOut(1, vdr.OUT_POOLED)]
    maps = [vdr.AttnMap(1, N, True), vdr.AttnMap(2, 1)]
    facets = [vdr.FacetOut(2, "key", 2), vdr.FacetOut(0, "value"), vdr.FacetOut(2, "token", 1, dtype=torch.bfloat16),
              vdr.FacetOut(1, "query", all_rows=True), vdr.FacetOut(2, "key"), vdr.FacetOut(0, "token", 3), vdr.FacetOut(2, "query", 3)]
    want_outs = e.forward_layers(x, outs)
    _, want_maps = e.forward_attn_maps(x, maps)
    want_facets, _, _ = e.forward_descriptors(x, facets)
    got_f, got_o, got_m = e.forward_descriptors(x, facets, outs=outs, maps=maps)
    for a, b in zip(got_o + got_m + got_f, want_outs + want_maps + want_facets):
        assert a.shape == b.shape and torch.equal(a, b)
    # ... and in another order, one facet at a time
    for k in (3, 0, 6, 2):
        (one,), _, _ = e.forward_descriptors(x, [facets[k]])
        assert torch.equal(one, want_facets[k]), k


# ---- 5. early stop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fold", "nofold", "fp8"])
def test_key_only_last_block_stops_after_its_qkv_gemm(path):
    import vdr
    w = vo.make_weights(P16, seed=3, scale=0.05)
    x = vo.make_images(P16, 4, seed=4).cuda()
    e = hc.engine(P16, w, **{"fold": {}, "nofold": dict(ln_fold=False), "fp8": dict(fp8=1)}[path])
    L = P16.layers
    e.profile(True)
    (key,), _, _ = e.forward_descriptors(x, [vdr.FacetOut(L - 1, "key")])
    a = e.profile_read()
    (key2, _), _, _ = e.forward_descriptors(x, [vdr.FacetOut(L - 1, "key"), vdr.FacetOut(L - 1, "token")])
    b = e.profile_read()
    e.profile(False)
    assert torch.equal(key, key2)
    assert a["gemm_qkv"]["launches"] == b["gemm_qkv"]["launches"] and b["gemm_qkv"]["launches"] % L == 0
    for cls in ("attention", "gemm_proj", "gemm_fc1", "gemm_fc2"):
        assert b[cls]["launches"] % L == 0 and a[cls]["launches"] == b[cls]["launches"] // L * (L - 1), (cls, a[cls], b[cls])
    assert "cls_tail" not in a and "cls_tail" not in b
    # with a map of that block the forward goes on through its attention, and no further
    e.profile(True)
    (key3,), _, _ = e.forward_descriptors(x, [vdr.FacetOut(L - 1, "key")], maps=[vdr.AttnMap(L - 1, 1)])
    c = e.profile_read()
    e.profile(False)
    assert torch.equal(key, key3)
    assert c["attention"]["launches"] == b["attention"]["launches"]
    for cls in ("gemm_proj", "gemm_fc1", "gemm_fc2"):
        assert c[cls]["launches"] == a[cls]["launches"], cls


# ---- 6. micro-batches ----------------------------------------------------------------------------------------------------
def test_micro_batches_write_their_own_rows():
    import vdr
    w = vo.make_weights(P16, seed=3, scale=0.05)
    x = vo.make_images(P16, 3, seed=4).cuda()
    req = [vdr.FacetOut(2, "key", 2), vdr.FacetOut(1, "value", all_rows=True), vdr.FacetOut(2, "token", 3, dtype=torch.bfloat16),
           vdr.FacetOut(0, "query", dtype=torch.bfloat16), vdr.FacetOut(1, "token")]
    want, _, _ = hc.engine(P16, w).forward_descriptors(x, req)
    for kw in (dict(micro_batch=2), dict(micro_batch=1, streams=2)):
        got, _, _ = hc.engine(P16, w, **kw).forward_descriptors(x, req)
        for a, b in zip(got, want):
            assert torch.equal(a, b), kw


# ---- 7. registers --------------------------------------------------------------------------------------------------------
def test_register_rows_are_prefix_rows():
    import vdr
    rc = dr.RegCfg(vo.VitCfg(32, 8, 3, 64, 1, 2, 128, layerscale=True), 4, False)
    w = dr.make_weights(rc, seed=5, scale=0.05)
    x = vo.make_images(rc.vit, 2, seed=6)
    e = vdr.Engine(dr.vdr_config(rc))
    e.load_weights(w)
    P, n = rc.n_prefix, rc.vit.n_patches
    assert P == 5 and e.n_tokens == n + 5
    ref, emu = dref.facets(rc, w, x), dref.facets(rc, w, x, emulate=True)
    for f in ("key", "token"):
        (rows, allr, binned), _, _ = e.forward_descriptors(x.cuda(), [vdr.FacetOut(1, f), vdr.FacetOut(1, f, all_rows=True), vdr.FacetOut(1, f, 1)])
        assert rows.shape == (2, n, 64) and allr.shape == (2, n + 5, 64)
        assert torch.equal(rows, allr[:, 5:])
        assert torch.equal(binned[:, :, 4 * 64:5 * 64], rows)
        check_parity(allr, ref[f][1], f"registers {f}.1", gate_l2(2), emu[f][1])


# ---- 8. DINOv3: before the rotation --------------------------------------------------------------------------------------
def test_dinov3_key_facet_is_taken_before_the_rotation():
    import vdr
    rc = hc.reg_cfg("dinov3_hf_tiny")
    assert rc.rope
    w = dr.make_weights(rc, seed=3, scale=0.05)
    x = vo.make_images(rc.vit, 2, seed=7)
    e = vdr.Engine(dr.vdr_config(rc))
    e.load_weights(w)
    ref, emu = dref.facets(rc, w, x), dref.facets(rc, w, x, emulate=True)
    L = rc.vit.layers
    maps = [vdr.AttnMap(L - 1, 1), vdr.AttnMap(0, e.n_tokens, True)]
    _, want_maps = e.forward_attn_maps(x.cuda(), maps)
    req = [vdr.FacetOut(i, f, all_rows=True) for i in range(L) for f in ("key", "query")]
    got, _, got_maps = e.forward_descriptors(x.cuda(), req, maps=maps)
    for r, t in zip(req, got):
        gl = gate_l2(r.layer + 1)
        check_parity(t, ref[r.facet][r.layer], f"dinov3 {r.facet}.{r.layer} (pre-rotation)", gl, emu[r.facet][r.layer])
    for a, b in zip(got_maps, want_maps):
        assert torch.equal(a, b)
    # (the rotated keys are a different tensor: the gate would not hold against them)
    P, dh = rc.n_prefix, rc.vit.dim // rc.vit.heads
    cos, sin = dr.rope_table(e.grid, dh, rc.rope_theta)
    k0 = ref["key"][0][:, P:].reshape(2, -1, rc.vit.heads, dh).transpose(1, 2)
    rot = dr.rotate(k0, cos, sin).transpose(1, 2).reshape(2, -1, rc.vit.dim)
    assert rel_l2(got[0][:, P:].float().cpu(), rot) > 10 * gate_l2(1)


# ---- 9. patch stride -----------------------------------------------------------------------------------------------------
def test_patch_stride_reshape_and_bin(monkeypatch):
    from vdr import ops
    w, x = _tiny()
    m = _model(monkeypatch, TINY, w)
    m.set_patch_stride(4)
    gh, gw = m.grid
    assert (gh, gw) == (7, 7)
    xd = x.cuda()
    d = m.extract_descriptors(xd, facet="key", bin=True, reshape=True)
    assert d.shape == (2, 7, 7, 17 * TINY.dim) and d.dtype == torch.float32
    flat = m.extract_descriptors(xd, facet="key")
    assert flat.shape == (2, 1, 49, TINY.dim)
    assert torch.equal(d.reshape(2, 49, -1), ops.log_bin(flat[:, 0].to(torch.bfloat16), 7, 7, 2, torch.float32))
    full = m.extract_descriptors(xd, layer=0, facet="token", include_cls=True)
    assert full.shape == (2, 1, 50, TINY.dim)
    d3 = m.extract_descriptors(xd, layer=0, facet="value", bin=True, hierarchy=3)
    assert d3.shape == (2, 1, 49, 25 * TINY.dim)


# ---- 10. the dense-descriptor entry points -------------------------------------------------------------------------------
def test_dense_descriptor_entry_points(monkeypatch):
    import vdr
    from vdr import pipeline
    cfg = vo.VitCfg(96, 16, 3, 128, 2, 2, 512)
    w = vo.make_weights(cfg, seed=11, scale=0.05)
    model = _model(monkeypatch, cfg, w, "_facet_b16")
    D = cfg.dim
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(12))
    xd = x.cuda()
    # defaults: the paths that were there, bit for bit
    d0 = vdr.get_dense_descriptor(model, x[0])
    assert d0.shape == (6, 6, D) and np.array_equal(d0, model.patch_embed(xd[:1]).cpu().numpy().reshape(6, 6, D))
    e0 = vdr.extract_dense(model, xd)
    assert np.array_equal(e0, model.engine.forward(xd, vdr.OUT_DENSE, torch.float32).reshape(2, 6, 6, D).cpu().numpy())
    # facets: the wider maps
    want = model.extract_descriptors(xd, facet="key", bin=True, reshape=True).cpu().numpy()
    dk = vdr.get_dense_descriptor(model, x[0], facet="key", bin=True)
    assert dk.shape == (6, 6, 17 * D) and dk.dtype == np.float32 and np.array_equal(dk, want[0])
    ek = vdr.extract_dense(model, xd, facet="key", bin=True)
    assert ek.shape == (2, 6, 6, 17 * D) and np.array_equal(ek, want)
    assert vdr.extract_dense(model, xd, facet="token", layer=0).shape == (2, 6, 6, D)
    # generate_features: the ROI crop on the wider channel count
    rng = np.random.default_rng(8)
    H, W, S = 72, 80, 2
    img = rng.random((H, W, S, 3)).astype(np.float32)
    mask = np.zeros((H, W, S), dtype=bool)
    mask[30:41, 36:50, :] = True
    f0, m0 = pipeline.generate_features(model, img, mask)
    fn, _ = pipeline.generate_features(model, img, mask, descriptor=None)
    fk, mk = pipeline.generate_features(model, img, mask, descriptor=dict(facet="key"))
    fb, mb = pipeline.generate_features(model, img, mask, descriptor=dict(facet="key", bin=True, hierarchy=2))
    assert len(f0) == len(fk) == len(fb) == S
    for i in range(S):
        assert np.array_equal(f0[i], fn[i])
        assert fk[i].shape == f0[i].shape and fb[i].shape == f0[i].shape[:2] + (17 * D,)
        assert np.array_equal(fb[i][:, :, 4 * D:5 * D], fk[i])  # bin 4 of level 0 is the patch itself
        assert np.array_equal(m0[i], mk[i]) and np.array_equal(m0[i], mb[i])


# ---- 11. a hierarchy whose level means do not fit is refused before anything is written ------------------------------------
def test_level_means_that_do_not_fit_are_refused_before_the_first_launch():
    """mlp_hidden = D: the fc1 activation buffer holds Mp * D bf16, the level means of h = 3 need 2 * B * n * D fp32 -- with
    batch 64 on a 4 x 4 grid 4 * 64 * 16 = 4096 rows' worth against Mp = 1536.  The call is refused (VDR_ERR_UNSUPPORTED) with
    no output of it written, the facets of earlier blocks included; h = 1 (no level means) and the un-binned facets still run."""
    import vdr
    cfg = vo.VitCfg(64, 16, 3, 128, 2, 2, 128)
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 64, seed=4).cuda()
    e = hc.engine(cfg, w)
    first = torch.full((64, cfg.n_patches, cfg.dim), -5.0, device="cuda")
    feat = torch.full((64, cfg.dim), -5.0, device="cuda")
    with pytest.raises(vdr.VdrError, match="do not fit") as ei:
        e.forward_descriptors(x, [vdr.FacetOut(0, "key", out=first), vdr.FacetOut(1, "key", 3)], outs=[vdr.LayerOut(0, vdr.OUT_CLS, out=feat)])
    assert ei.value.code == -7
    torch.cuda.synchronize()
    assert torch.all(first == -5.0) and torch.all(feat == -5.0)
    (a, b), _, _ = e.forward_descriptors(x, [vdr.FacetOut(0, "key", out=first), vdr.FacetOut(1, "key", 1)])
    assert a is first and not torch.any(first == -5.0) and b.shape == (64, cfg.n_patches, 9 * cfg.dim)
