"""GPU: the SAM / MedSAM encoder at other input sizes -- the rel-pos resampling kernel, global attention over any g x g
grid (g <= 64: the run-time-grid kernel), native-shape tables through vdr_set_weight / vdr_finalize, load_model(img_size=).

References and gates are the existing ones: the float64 attention reference and tolerances of test_attention_relpos_windows
(tests/test_ops_gpu.py), the gates of test_sam_encoder_small / test_sam_encoder_fp8 / test_sam_golden_transformers_crosscheck
(tests/test_model_gpu.py) and of test_medsam_vit_b_1024_all_twelve_blocks (tests/test_fullsize_gpu.py), against the UNCHANGED
oracle fed tables resampled on the host in float64 (vdr.weights.sam_tables_at; checked against transformers on the CPU in
tests/test_sam_size_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import handle_configs as hc
from fixtures import ops  # noqa: F401
from model_gates import check_batch_properties, check_parity, check_parity_fp8, gate_l2, gate_l2_fp8, min_cos, rel_l2
from ops_checks import BF16_EPS, assert_close, assert_unbiased, bf, relpos_attn_ref
from oracle import sam_oracle as so
from sam_size_ref import golden_cases, linear_def, within_half_ulp

pytestmark = pytest.mark.gpu


# ---- 1. the resampling kernel -----------------------------------------------------------------------------------
def test_interpolate_rel_pos_kernel(ops):
    from vdr.weights import interpolate_rel_pos
    gen = torch.Generator().manual_seed(7)
    # integer tables, dyadic weights: exact
    for L0, L in ((26, 13), (28, 7), (8, 16), (5, 20), (127, 127)):
        t = torch.randint(-64, 64, (L0, 64), generator=gen).float()
        got = ops.interpolate_rel_pos(t.cuda(), L).cpu()
        assert got.shape == (L, 64) and got.dtype == torch.float32
        assert np.array_equal(got.double().numpy(), linear_def(t, L)), (L0, L)
    # random tables at SAM lengths, channel counts that are no multiple of the workgroup: half an fp32 ulp of the float64
    # definition, and the host statement of it
    for g0, g, D in ((64, 32, 64), (64, 16, 64), (64, 48, 64), (14, 9, 64), (14, 20, 64), (10, 15, 64), (7, 64, 64), (64, 1, 64),
                     (1, 5, 64), (64, 33, 80), (14, 57, 3)):
        t = torch.randn(2 * g0 - 1, D, generator=gen)
        got = ops.interpolate_rel_pos(t.cuda(), 2 * g - 1).cpu()
        assert within_half_ulp(got, linear_def(t, 2 * g - 1)), (g0, g, D)
        host = interpolate_rel_pos(t, 2 * g - 1)
        assert float((got - host).abs().max()) <= float(np.spacing(np.float32(t.abs().max()))), (g0, g, D)


# ---- 2. global attention at any grid side -----------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H", [(2, 5, 2), (3, 9, 1), (2, 12, 2), (2, 20, 3), (1, 33, 2), (1, 48, 1), (1, 57, 2), (2, 32, 12),
                                   (3, 1, 2), (2, 16, 2), (1, 63, 1)])
def test_attention_relpos_any_grid_side(ops, B, S, H):
    g = torch.Generator().manual_seed(S * 100 + B)
    qkv = bf(torch.randn(B * S * S, 3 * H * 64, generator=g))
    rel_h = torch.randn(2 * S - 1, 64, generator=g) * 0.1
    rel_w = torch.randn(2 * S - 1, 64, generator=g) * 0.1
    ref = relpos_attn_ref(qkv, rel_h, rel_w, B, S, H)
    out = ops.attention_relpos(qkv.cuda(), rel_h.cuda(), rel_w.cuda(), B, S, H)
    assert_close(out, ref, 2 * BF16_EPS, 6e-3, f"relpos attention B{B} S{S} H{H}")
    assert_unbiased(out, ref, f"relpos attention B{B} S{S} H{H}")


# ---- 3. a designed input that must come out bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("g,s,t", [(9, 2, 5), (20, 7, 0), (33, 1, 32), (57, 30, 11), (64, 63, 1), (12, 0, 0), (48, 47, 24)])
def test_attention_relpos_designed_shift_is_exact(ops, g, s, t):
    """k = 0, q = 16 (e0 + e1) in every row, rel_pos_h = 8 in channel 0 at the two rows that stand for kh = (qh + s) mod g,
    rel_pos_w likewise in channel 1 for kw = (qw + t) mod g: the key ((qh + s) mod g, (qw + t) mod g) has logit 256, every
    other key 128 or 0, exp(-128) is 0 in fp32, so output row (qh, qw) IS that v row.  Exercises the run-time key -> (kh, kw)
    arithmetic across chunk boundaries, the ragged last chunk and the rescaling of the online softmax."""
    B, H = 2, 2
    gen = torch.Generator().manual_seed(g * 1000 + s * 10 + t)
    n = g * g
    qkv = torch.zeros(B, n, 3, H, 64)
    qkv[:, :, 0, :, 0] = 16.0
    qkv[:, :, 0, :, 1] = 16.0
    v = torch.randint(1, 9, (B, n, H, 64), generator=gen).float() * (torch.randint(0, 2, (B, n, H, 64), generator=gen) * 2 - 1).float()
    qkv[:, :, 2] = v
    rel_h, rel_w = torch.zeros(2 * g - 1, 64), torch.zeros(2 * g - 1, 64)
    for tab, ch, sh in ((rel_h, 0, s), (rel_w, 1, t)):
        for row in (g - 1 - sh, 2 * g - 1 - sh):
            if 0 <= row < 2 * g - 1:
                tab[row, ch] = 8.0
    out = ops.attention_relpos(qkv.reshape(B * n, 3 * H * 64).to(torch.bfloat16).cuda(), rel_h.cuda(), rel_w.cuda(), B, g, H)
    qh, qw = torch.arange(n) // g, torch.arange(n) % g
    target = ((qh + s) % g) * g + (qw + t) % g
    want = v[:, target].reshape(B * n, H * 64)
    assert torch.equal(out.float().cpu(), want), (g, s, t)


# ---- 4. small models at other sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(7))
def test_sam_small_models_at_other_sizes(golden_dir, n):
    """The transformers fixtures' models, native tables loaded as they are into an encoder built at another size: tokens and
    neck output against the fp32 and the bf16-emulating oracle (host-resampled tables) at test_sam_encoder_small's gates,
    and the neck output against transformers at test_sam_golden_transformers_crosscheck's."""
    import vdr
    from vdr.weights import sam_tables_at
    cn, cs, batch, wseed, xseed, wscale, want = golden_cases(golden_dir)[n]
    w0 = so.make_weights(cn, seed=wseed, scale=wscale)
    ws = sam_tables_at(w0, cs.grid, cs.global_idx)
    x = so.make_images(cs, batch, seed=xseed)
    ref = so.sam_forward(cs, ws, x)
    emu = so.sam_forward(cs, ws, x, emulate_bf16=True)
    e = hc.sam_engine(cs, w0)  # NATIVE tables: pos_embed [1, g0, g0, D], rel_pos [2 g0 - 1, 64] in the global blocks
    g = cs.grid
    name = f"{cn.img} -> {cs.img}"
    tok = e.forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity(tok, ref["tokens"].reshape(batch, g * g, cs.dim), f"sam {name} tokens", gate_l2(cs.layers),
                 emu["tokens"].reshape(batch, g * g, cs.dim))
    out = e.forward(x.cuda(), vdr.OUT_ENCODER)
    assert out.shape == (batch, g, g, cs.out_chans)
    check_parity(out, ref["out"].permute(0, 2, 3, 1), f"sam {name} neck output", gate_l2(cs.layers) + 4e-3,
                 emu["out"].permute(0, 2, 3, 1))
    got = out.permute(0, 3, 1, 2)[:, :want.shape[1]].cpu()
    r, c = rel_l2(got, want), min_cos(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1))
    print(f"sam {name} vs transformers: relL2 {r:.3e} min cos {c:.6f}")
    assert r <= gate_l2(cs.layers) + 4e-3
    assert c >= 0.999
    # the device resampling is the host definition: a handle given the host-resampled tables computes the same bits
    assert torch.equal(out, hc.sam_engine(cs, ws).forward(x.cuda(), vdr.OUT_ENCODER))


@pytest.mark.parametrize("n", [2, 4])
def test_sam_small_models_at_other_sizes_fp8(golden_dir, n):
    import vdr
    from vdr.weights import sam_tables_at
    cn, cs, _, wseed, xseed, wscale, _ = golden_cases(golden_dir)[n]
    batch = 2
    w0 = so.make_weights(cn, seed=wseed, scale=wscale)
    ws = sam_tables_at(w0, cs.grid, cs.global_idx)
    x = so.make_images(cs, batch, seed=xseed)
    ref = so.sam_forward(cs, ws, x)
    emx = so.sam_forward(cs, ws, x, emulate_bf16="mx")
    e = hc.sam_engine(cs, w0, fp8=1)
    g = cs.grid
    tok = e.forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity_fp8(tok, ref["tokens"].reshape(batch, g * g, cs.dim), emx["tokens"].reshape(batch, g * g, cs.dim), cs.layers,
                     f"sam fp8 {cn.img} -> {cs.img} tokens")
    out = e.forward(x.cuda(), vdr.OUT_ENCODER)
    check_parity_fp8(out, ref["out"].permute(0, 2, 3, 1), emx["out"].permute(0, 2, 3, 1), cs.layers,
                     f"sam fp8 {cn.img} -> {cs.img} neck output")
    assert torch.equal(out, e.forward(x.cuda(), vdr.OUT_ENCODER))


# ---- 5. the native size is today's path, bit for bit ------------------------------------------------------------------
def test_native_checkpoint_at_its_native_size_is_bitwise_unchanged():
    import vdr
    cfg = so.SamCfg(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64)
    w = so.make_weights(cfg, seed=21, scale=0.05)
    x = so.make_images(cfg, 2, seed=22).cuda()
    plain = hc.sam_engine(cfg, w).forward(x, vdr.OUT_ENCODER)
    # a handle that was first given tables of ANOTHER native grid (kept for resampling), then the ones of its own shape:
    # the loaded tables themselves are used, no resampling step
    other = so.make_weights(hc.sized_sam(cfg, 320), seed=5, scale=0.05)
    e = vdr.Engine(hc.sam_config(cfg))
    e.load_weights({**w, "pos_embed": other["pos_embed"], "blocks.1.attn.rel_pos_h": other["blocks.1.attn.rel_pos_h"],
                    "blocks.1.attn.rel_pos_w": other["blocks.1.attn.rel_pos_w"]})
    assert not torch.equal(plain, e.forward(x, vdr.OUT_ENCODER))
    e.load_weights(w)
    assert torch.equal(plain, e.forward(x, vdr.OUT_ENCODER))


# ---- 6. full ViT-B geometry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [256, 512, 768])
def test_medsam_vit_b_geometry_at_other_sizes(side):
    """SAM ViT-B geometry (768 / 12 heads, window 14, global attention over the whole grid) with a native 1024^2 checkpoint
    -- pos_embed [1, 64, 64, 768], rel_pos [127, 64] -- loaded into an encoder built at 256^2 / 512^2 / 768^2, the depth cut
    to (window, window, global) so that the CPU oracle stays in seconds."""
    import vdr
    from vdr.weights import sam_tables_at
    cn = so.SamCfg(layers=3, global_idx=(2,))
    cs = hc.sized_sam(cn, side)
    g = cs.grid
    w0 = so.make_weights(cn, seed=23)
    assert tuple(w0["pos_embed"].shape) == (1, 64, 64, 768) and tuple(w0["blocks.2.attn.rel_pos_h"].shape) == (127, 64)
    ws = sam_tables_at(w0, g, cs.global_idx)
    B = 2
    x = so.make_images(cs, B, seed=24)
    ref = so.sam_forward(cs, ws, x)
    emu = so.sam_forward(cs, ws, x, emulate_bf16=True)
    vc = vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "img": side, "layers": 3, "global_blocks": (2,)})
    model = vdr.VitDescriptorModel(vc, w0, "medsam", sized=True)
    enc = model.image_encoder(x.cuda())
    assert enc.shape == (B, 256, g, g)
    check_parity(enc.permute(0, 2, 3, 1), ref["out"].permute(0, 2, 3, 1), f"ViT-B geometry at {side}^2 neck output",
                 gate_l2(3) + 4e-3, emu["out"].permute(0, 2, 3, 1))
    tok = model.engine.forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity(tok, ref["tokens"].reshape(B, g * g, 768), f"ViT-B geometry at {side}^2 tokens", gate_l2(3),
                 emu["tokens"].reshape(B, g * g, 768))
    # a raw gray slice goes straight to the model's side (one skimage-semantics resize, not 1024 first)
    from oracle import prep_oracle as po
    raw = np.random.default_rng(side).random((300, 280)).astype(np.float32)
    f = vdr.get_dense_descriptor(model, raw)
    assert f.shape == (g, g, 256) and f.dtype == np.float32
    direct = torch.from_numpy(po.prepare_image(raw, side=side))[None]
    want = so.sam_forward(cs, ws, direct)["out"][0].permute(1, 2, 0)
    check_parity(torch.from_numpy(f), want, f"get_dense_descriptor at {side}^2", gate_l2(3) + 4e-3, want)
    # a prepared image of the model's side is taken as it is
    np.testing.assert_array_equal(vdr.get_dense_descriptor(model, x[0].numpy()), np.transpose(enc[0].cpu().numpy(), (1, 2, 0)))


@pytest.mark.parametrize("fp8", [0, 1])
def test_medsam_vit_b_512_all_twelve_blocks(fp8):
    """load_model('medsam', img_size=512): the whole SAM ViT-B image encoder (12 blocks, global blocks 2 / 5 / 8 / 11 over
    32 x 32 tokens) with the native 1024^2 tables, at test_medsam_vit_b_1024_all_twelve_blocks's gates."""
    import vdr
    from vdr.weights import sam_tables_at
    cn = so.SAM_VIT_B
    cs = hc.sized_sam(cn, 512)
    w0 = so.make_weights(cn, seed=1)
    x = so.make_images(cs, 1, seed=3)
    ref = so.sam_forward(cs, sam_tables_at(w0, 32, cs.global_idx), x)["out"].permute(0, 2, 3, 1)
    m = vdr.load_model("medsam", weights=w0, img_size=512, fp8=fp8)
    assert m.cfg.img == 512 and m.engine.grid == (32, 32) and m.sized
    got = m.engine.forward(x.cuda(), vdr.OUT_ENCODER, torch.float32)
    assert got.shape == (1, 32, 32, 256)
    if fp8:
        check_parity(got, ref, "MedSAM 512^2 L=12 MX-fp8 neck output", gate_l2_fp8(12), cos=0.99)
    else:
        check_parity(got, ref, "MedSAM 512^2 L=12 neck output", gate_l2(12))
    xb = torch.cat([x, so.make_images(cs, 2, seed=4)]).cuda()
    outb = m.engine.forward(xb, vdr.OUT_ENCODER, torch.float32)
    assert torch.equal(outb[0], got[0])
    f = vdr.get_dense_descriptor(m, np.random.default_rng(1).random((200, 200)).astype(np.float32))
    assert f.shape == (32, 32, 256)


# ---- 7. batch properties at a new size ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [0, 1])
def test_batch_properties_at_a_new_size(fp8):
    import vdr
    cn = so.SamCfg(img=224, patch=16, dim=128, heads=2, layers=3, mlp_hidden=256, window=7, global_idx=(0, 2), out_chans=64)
    cs = hc.sized_sam(cn, 288)  # grid 18: padded windows, 324 tokens = 2 full key chunks + a ragged one
    w0 = so.make_weights(cn, seed=31, scale=0.05)
    e = hc.sam_engine(cs, w0, fp8=fp8)
    x = so.make_images(cs, 6, seed=32)
    x[5] = x[1]
    x = x.cuda()
    out = check_batch_properties(lambda t: e.forward(t, vdr.OUT_ENCODER), x, small=1, perm=[3, 0, 5, 2, 4, 1], lo=2)
    assert torch.equal(hc.sam_engine(cs, w0, fp8=fp8, micro_batch=4).forward(x, vdr.OUT_ENCODER), out)


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------
def test_forward_at_a_new_size_is_graph_capturable():
    """vdr_finalize did the resampling: the first forward of a handle loaded with native-shape tables neither allocates nor
    synchronises, and its replay reproduces an eager forward bit for bit."""
    import vdr
    cn = so.SamCfg(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64)
    cs = hc.sized_sam(cn, 176)
    w0 = so.make_weights(cn, seed=41, scale=0.05)
    x = so.make_images(cs, 3, seed=42).cuda()
    e = hc.sam_engine(cs, w0)
    out = torch.empty((3, 11, 11, 64), dtype=torch.float32, device="cuda")
    e._workspace(3)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            e.forward_into(x, out, vdr.OUT_ENCODER)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, hc.sam_engine(cs, w0).forward(x, vdr.OUT_ENCODER))


# ---- 9. generate_features takes the side and the grid from the model -----------------------------------------------------------
def test_generate_features_at_a_reduced_geometry():
    import vdr
    from oracle import prep_oracle as po
    from vdr import pipeline, prep
    from vdr.weights import sam_tables_at
    cn = so.SamCfg(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64)
    cs = hc.sized_sam(cn, 144)
    w0 = so.make_weights(cn, seed=21)
    model = vdr.VitDescriptorModel(hc.sam_config(cs), w0, "medsam", torch.device("cuda"), sized=True)
    rng = np.random.default_rng(8)
    H, W, S = 72, 80, 5
    img = rng.random((H, W, S)).astype(np.float32)
    mask = np.zeros((H, W, S), dtype=bool)
    mask[30:41, 36:50, 1:4] = True
    feats, masks = pipeline.generate_features(model, img, mask, max_batch=3)
    one, masks1 = pipeline.generate_features(model, img, mask, max_batch=1)  # slice by slice
    assert len(feats) == len(one) == S
    bigger = mask.sum(-1) > 0
    xmin, ymin, xmax, ymax = po.extract_coords(bigger, 2)
    c = max(xmax - xmin, ymax - ymin) * 2
    xm, ym = int(xmin + (xmax - xmin) / 2), int(ymin + (ymax - ymin) / 2)
    box = (xm - c, ym - c, xm + c, ym + c)
    img_c, big_c = po.crop_image(img, *box), po.crop_image(bigger, *box)
    ws = sam_tables_at(w0, cs.grid, cs.global_idx)
    for i in range(S):
        assert np.array_equal(feats[i], one[i]) and np.array_equal(masks[i], masks1[i]), i
        # ... which is the encoder run on that one slice prepared at the model's side
        xi = prep.prepare_slices(torch.from_numpy(img_c[:, :, i:i + 1]), side=144, out_dtype=torch.bfloat16, device=model.device)
        whole = model.engine.forward(xi, vdr.OUT_ENCODER, torch.float32)[0].cpu().numpy()
        assert whole.shape == (9, 9, 64)
        assert np.array_equal(feats[i], po.extract_roi(whole, big_c)), i
        f = so.sam_forward(cs, ws, torch.from_numpy(po.prepare_image(img_c[:, :, i], side=144))[None])["out"][0].permute(1, 2, 0).numpy()
        want = po.extract_roi(f, big_c)
        assert feats[i].shape == want.shape
        rel = np.linalg.norm(feats[i] - want) / np.linalg.norm(want)
        assert rel < 2e-2, (i, rel)


# ---- 10. refusals on a live handle ------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import vdr
    base = vdr.ARCHS["medsam"].__dict__
    with pytest.raises(vdr.VdrError) as ei:
        vdr.Engine(vdr.VdrConfig(**{**base, "img": 1040, "layers": 3, "global_blocks": (2,)}))
    assert ei.value.code == -7 and "at most 64" in str(ei.value)
    sam = vdr.Engine(vdr.VdrConfig(**{**base, "img": 512, "layers": 2, "global_blocks": (1,)}))
    assert sam.lib.vdr_set_input_size(sam.h, 256, 256) == -7  # VDR_ERR_UNSUPPORTED: the size is a load-time property
    assert b"SAM" in sam.lib.vdr_last_error(sam.h)
    need = C.c_size_t()
    assert sam.lib.vdr_workspace_bytes(sam.h, 2, 0, C.byref(need)) == 0
    big = vdr.Engine(vdr.VdrConfig(**{**base, "layers": 2, "global_blocks": (1,)}))
    need1024 = C.c_size_t()
    assert big.lib.vdr_workspace_bytes(big.h, 2, 0, C.byref(need1024)) == 0
    assert 0 < need.value < need1024.value / 3  # the workspace is that of the handle's own size

    def set_weight(e, name, shape):
        a = np.zeros(shape, dtype=np.float32)
        sh = (C.c_int64 * a.ndim)(*a.shape)
        return e.lib.vdr_set_weight(e.h, name.encode(), a.ctypes.data_as(C.c_void_p), sh, a.ndim)
    assert set_weight(sam, "pos_embed", (1, 64, 64, 768)) == 0          # native 1024^2 table
    assert set_weight(sam, "pos_embed", (1, 32, 32, 768)) == 0          # the handle's own shape
    assert set_weight(sam, "blocks.1.attn.rel_pos_h", (127, 64)) == 0
    assert set_weight(sam, "blocks.1.attn.rel_pos_w", (27, 64)) == 0
    for name, shape in (("pos_embed", (1, 64, 64, 384)), ("pos_embed", (1, 65, 65, 768)), ("pos_embed", (1, 64, 32, 768)),
                        ("pos_embed", (64 * 64, 768)), ("blocks.1.attn.rel_pos_h", (128, 64)), ("blocks.1.attn.rel_pos_h", (129, 64)),
                        ("blocks.1.attn.rel_pos_h", (127, 32)), ("blocks.0.attn.rel_pos_h", (127, 64)),  # a window block
                        ("blocks.0.norm1.weight", (1, 32, 32, 768))):
        assert set_weight(sam, name, shape) == -1, (name, shape)
        assert b"expected" in sam.lib.vdr_last_error(sam.h)
    vit = vdr.Engine(vdr.ARCHS["vit_base16_224"])
    assert set_weight(vit, "pos_embed", (1, 10, 10, 768)) == -1  # plain ViTs: vdr_set_input_size
