"""GPU: ViT / DINOv2 models at input sizes other than the one pos_embed was learned at (vdr_set_input_size).

The definition every check uses: the patch rows of the position table are F.interpolate(table.double(), size=(gh, gw),
mode="bicubic", align_corners=False) rounded to fp32 once (vdr.weights.interpolate_pos_embed); the UNCHANGED oracle fed
that table is the reference for the models (tests/test_input_size_cpu.py ties it to transformers).  Model gates are the
project's own (tests/model_gates.py): min row cosine >= 0.999 and rel-L2 <= 4e-3 + 3e-3 sqrt(L) against the fp32 and the
bf16-emulating oracle; fp8 with check_parity_fp8's levels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
from model_gates import check_batch_properties, check_parity, check_parity_fp8, gate_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


# ---- helpers ------------------------------------------------------------------------------------------------
def _engine(cfg, w, size=None, layers=None, **kw):
    """An engine of cfg's weights (truncated to `layers` blocks), told `size` = (H, W) when given."""
    L = cfg.layers if layers is None else layers
    e = hc.engine(cfg, hc.first_blocks(w, L), layers=L, **kw)
    if size is not None:
        e.set_input_size(*size)
    return e


def _images(batch, H, W, seed, chans=3):
    """[0, 1) pixels that bf16 holds exactly: fp32 and bf16 pixel buffers then carry the same values."""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    x = torch.from_numpy(rng.random(size=(batch, chans, H, W), dtype=np.float32))
    return x.to(torch.bfloat16).float()


def _weights_at(cfg, w, size):
    """The weights the oracle gets at `size`: pos_embed resampled in float64, rounded once."""
    from vdr.weights import interpolate_pos_embed
    ws = dict(w)
    if cfg.has_pos:
        ws["pos_embed"] = interpolate_pos_embed(w["pos_embed"], (size[0] // cfg.patch, size[1] // cfg.patch), 1 if cfg.has_cls else 0)
    return ws


def _sizes(cfg):
    """a larger square, a smaller square, both rectangular orientations"""
    s = cfg.img
    return [(2 * s, 2 * s), (s // 2, s // 2), (3 * s // 4, 3 * s // 2), (3 * s // 2, 3 * s // 4)]


SMALL = {  # tests/test_model_gpu.py
    "tiny_p8": hc.TINY,
    "p16_d128": vo.VitCfg(64, 16, 3, 128, 2, 3, 512),
    "p14_d192": vo.VitCfg(56, 14, 3, 192, 3, 2, 768),
    "dinov2_swiglu_ls": vo.VitCfg(56, 14, 3, 128, 2, 2, 320 + 64, act="swiglu", layerscale=True),
}


# ---- 1. the kernel -----------------------------------------------------------------------------------------
def _interp64(t, g0, g):
    """float64 definition, NOT rounded: t [g0h*g0w, D] -> double [gh*gw, D]"""
    D = t.shape[1]
    p = t.double().reshape(1, g0[0], g0[1], D).permute(0, 3, 1, 2)
    p = torch.nn.functional.interpolate(p, size=tuple(g), mode="bicubic", align_corners=False)
    return p.permute(0, 2, 3, 1).reshape(g[0] * g[1], D)


@pytest.mark.parametrize("g0,g", [((6, 6), (12, 12)), ((12, 12), (6, 6)), ((5, 7), (20, 14)), ((9, 9), (9, 9)), ((16, 16), (32, 32))])
def test_interpolate_pos_integer_tables_are_exact(g0, g):
    """Integer tables (|v| <= 8) at ratios 2x, 1/2x, 4x2 and 1x: every cubic weight is a dyadic rational there, so the
    float64 definition is exact in any summation order and the kernel must give its bits."""
    from vdr import ops
    gen = torch.Generator().manual_seed(g0[0] * 100 + g[1])
    t = torch.randint(-8, 9, (g0[0] * g0[1], 96), generator=gen).float()
    ref = _interp64(t, g0, g)
    assert torch.equal(ref, ref.float().double())  # (exactly representable: one rounding changes nothing)
    got = ops.interpolate_pos(t.cuda(), g0, g).cpu()
    assert torch.equal(got, ref.float())
    if g0 == g:
        assert torch.equal(got, t)
    else:
        assert (ref != ref.round()).any()  # (the taps do mix: not a copy)


@pytest.mark.parametrize("D", [64, 384, 1536])
@pytest.mark.parametrize("g0,g", [((37, 37), (64, 64)), ((16, 16), (24, 40)), ((14, 14), (16, 16)), ((4, 4), (7, 5))])
def test_interpolate_pos_random_tables_within_half_an_ulp(g0, g, D):
    """|got - ref64| <= 2^-24 |ref64| + 2^-40 max|table|: half an fp32 ulp for the kernel's single rounding; the second
    term covers the fp64 summation order under cancellation.  Derived, not measured: a kernel that evaluates anything
    in fp32 (as torch's own fp32 path, which rounds the source coordinate) misses it by orders of magnitude."""
    from vdr import ops
    gen = torch.Generator().manual_seed(D + g0[0] + g[1])
    t = torch.randn(g0[0] * g0[1], D, generator=gen) * 0.02
    ref = _interp64(t, g0, g)
    got = ops.interpolate_pos(t.cuda(), g0, g).cpu().double()
    bound = 2.0 ** -24 * ref.abs() + 2.0 ** -40 * t.abs().max().double()
    excess = ((got - ref).abs() / bound).max().item()
    print(f"interpolate_pos {g0}->{g} D={D}: max |got - ref64| / bound = {excess:.3f}")
    assert excess <= 1.0
    # the check can see an fp32 evaluation: torch's fp32 path on the same table breaks the bound
    if g0 == (37, 37):
        f32 = torch.nn.functional.interpolate(t.reshape(1, 37, 37, D).permute(0, 3, 1, 2), size=tuple(g), mode="bicubic",
                                              align_corners=False).permute(0, 2, 3, 1).reshape(g[0] * g[1], D).double()
        assert ((f32 - ref).abs() / bound).max().item() > 1.0


# ---- 2. round trip -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p16_d128", "dinov2_swiglu_ls"])
def test_native_other_native_is_bitwise_a_fresh_engine(name):
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 5, seed=4).cuda()
    fresh = _engine(cfg, w)
    want = {m: fresh.forward(x, m) for m in (vdr.OUT_CLS, vdr.OUT_DENSE)}
    e = _engine(cfg, w)
    assert e.input_size == (cfg.img, cfg.img)
    hh, ww = C.c_int(), C.c_int()
    for size in _sizes(cfg):
        e.set_input_size(*size)
        assert e.lib.vdr_get_input_size(e.h, C.byref(hh), C.byref(ww)) == 0 and (hh.value, ww.value) == size == e.input_size
        xs = _images(2, *size, seed=1).cuda()
        assert e.forward(xs, vdr.OUT_DENSE).shape == (2, (size[0] // cfg.patch) * (size[1] // cfg.patch), cfg.dim)
        with pytest.raises(ValueError, match="images must be"):
            e.forward(x, vdr.OUT_CLS)  # the native shape is refused while another size is in force
        e.set_input_size(cfg.img, cfg.img)
        for m, t in want.items():
            assert torch.equal(e.forward(x, m), t), (name, size, m)


# ---- 3. models vs the oracle ---------------------------------------------------------------------------------
SWITCHES = {
    "default": dict(),
    "no_ln_fold": dict(ln_fold=False),
    "resid_fp32": dict(resid_fp32=True),
    "micro_batch": dict(micro_batch=2),
    "streams": dict(micro_batch=2, streams=2),
    "ln_fin_fused": dict(ln_fin_fused=True),
    "full_last_block": dict(full_last_block=True),
    "fp8": dict(fp8=1),
    "fp8_cls_bf16": dict(fp8=1, fp8_cls_bf16=True),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_models_at_other_sizes(name, switch):
    """CLS / DENSE / TOKENS / PATCH_EMBED at a larger square, a smaller square and both rectangular orientations, fp32 and
    bf16 pixels (the gathered and the im2col patch paths), one engine moved from size to size."""
    import vdr
    cfg = SMALL[name]
    kw = SWITCHES[switch]
    fp8 = bool(kw.get("fp8"))
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    e = _engine(cfg, w, **kw)
    g = gate_l2(cfg.layers)
    B = 5
    for k, size in enumerate(_sizes(cfg)):
        x = _images(B, *size, seed=10 + k)
        ws = _weights_at(cfg, w, size)
        ref = vo.forward_images(cfg, ws, x)
        emu = vo.forward_images(cfg, ws, x, emulate_bf16="mx" if fp8 else True)
        e.set_input_size(*size)
        n = (size[0] // cfg.patch) * (size[1] // cfg.patch)
        assert e.n_patches == n and ref["dense"].shape == (B, n, cfg.dim)
        for dt in (torch.float32, torch.bfloat16):
            xd = x.cuda().to(dt)
            tag = f"{name} {switch} {size[0]}x{size[1]} {'bf16' if dt == torch.bfloat16 else 'fp32'} pixels"
            for mode, key in ((vdr.OUT_CLS, "cls"), (vdr.OUT_DENSE, "dense"), (vdr.OUT_TOKENS, "tokens")):
                if fp8:
                    check_parity_fp8(e.forward(xd, mode), ref[key], emu[key], cfg.layers, f"{tag} {key}")
                else:
                    check_parity(e.forward(xd, mode), ref[key], f"{tag} {key}", g, emu[key])
            pe_emu = vo.forward_images(cfg, ws, x, emulate_bf16=True)["patch_embed"] if fp8 else emu["patch_embed"]
            check_parity(e.forward(xd, vdr.OUT_PATCH_EMBED), ref["patch_embed"], f"{tag} patch_embed", 4e-3, pe_emu)


# ---- 4. token counts across the attention launcher's classes -----------------------------------------------------
@pytest.mark.parametrize("size,N", [((64, 64), 17), ((160, 176), 111), ((224, 208), 183), ((256, 256), 257), ((320, 320), 401)])
def test_token_counts_across_the_attention_classes(size, N):
    """<= 64, <= 128, <= 224, <= 288, > 288 tokens: one small p = 16 model (native 96^2) at five sizes."""
    import vdr
    cfg = vo.VitCfg(96, 16, 3, 128, 2, 2, 512)
    w = vo.make_weights(cfg, seed=8, scale=0.05)
    x = _images(3, *size, seed=9)
    ws = _weights_at(cfg, w, size)
    assert ws["pos_embed"].shape[1] == N
    ref = vo.forward_images(cfg, ws, x)
    emu = vo.forward_images(cfg, ws, x, emulate_bf16=True)
    e = _engine(cfg, w, size)
    assert e.n_tokens == N
    g = gate_l2(cfg.layers)
    for dt in (torch.float32, torch.bfloat16):
        for mode, key in ((vdr.OUT_CLS, "cls"), (vdr.OUT_TOKENS, "tokens")):
            check_parity(e.forward(x.cuda().to(dt), mode), ref[key], f"N={N} {size} {dt} {key}", g, emu[key])


# ---- 5. the transformers fixtures on the device -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["dinov2_hf_resize", "vit_hf_resize"])
def test_transformers_fixtures_at_other_sizes(golden_dir, name):
    import vdr
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    sw = name.startswith("dinov2")
    cfg = vo.VitCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]),
                    act="swiglu" if sw else "gelu", layerscale=sw, ln_eps=1e-6)
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    e = _engine(cfg, w)
    gl = gate_l2(cfg.layers)
    for k, (H, W) in enumerate([tuple(int(v) for v in s) for s in g["sizes"]]):
        x = torch.rand((int(g["batch"]), 3, H, W), generator=torch.Generator().manual_seed(int(g["xseed"]) + k), dtype=torch.float32)
        want = torch.from_numpy(g[f"tokens_{H}x{W}"])
        emu = vo.forward_images(cfg, _weights_at(cfg, w, (H, W)), x, emulate_bf16=True)["tokens"]
        e.set_input_size(H, W)
        check_parity(e.forward(x.cuda(), vdr.OUT_TOKENS), want, f"{name} {H}x{W} tokens", gl, emu)


# ---- 6. the DINOv2-style outputs at a rectangular size ------------------------------------------------------------
def test_layers_maps_and_dynamic_size_at_a_rectangular_size():
    import vdr
    from vdr.model import VitDescriptorModel
    cfg = vo.VitCfg(56, 14, 3, 128, 2, 3, 320 + 64, act="swiglu", layerscale=True)
    size, (gh, gw) = (84, 42), (6, 3)
    N = gh * gw + 1
    w = vo.make_weights(cfg, seed=21, scale=0.05)
    x = _images(4, *size, seed=22).cuda()
    full = _engine(cfg, w, size)
    modes = (vdr.OUT_CLS, vdr.OUT_DENSE, vdr.OUT_TOKENS)
    specs = [vdr.LayerOut(i, m, dt) for i in range(cfg.layers) for m in modes for dt in (torch.float32, torch.bfloat16)]
    got = full.forward_layers(x, specs)
    for i in range(cfg.layers):
        trunc = _engine(cfg, w, size, layers=i + 1)
        for sp, t in zip(specs, got):
            if sp.layer == i:
                assert torch.equal(t, trunc.forward(x, sp.mode, sp.dtype)), (i, sp.mode, sp.dtype)
    assert not torch.equal(got[0], got[6])
    # attention maps follow N' and (gh, gw); rows sum to 1 (tests/test_attn_maps_gpu.py: atol 1e-5)
    static = VitDescriptorModel(hc.vit_config(cfg), w).set_input_size(*size)
    dyn = VitDescriptorModel(hc.vit_config(cfg), w, dynamic_size=True)
    assert static.input_size == size and static.grid == (gh, gw) and dyn.input_size == (56, 56)
    last = static.get_last_selfattention(x)
    assert last.shape == (4, cfg.heads, N, N)
    assert torch.allclose(last.sum(-1), torch.ones(4, cfg.heads, N, device=last.device), atol=1e-5)
    heat = static.get_attention_maps(x, layers=[0, 2], cls_only=True, reshape=True)
    assert all(t.shape == (4, cfg.heads, gh, gw) for t in heat)
    assert static.get_attention_maps(x, head_mean=True).shape == (4, N)
    # dynamic_size adopts x.shape[-2:]: the same tensors as the explicit call
    assert torch.equal(dyn.get_last_selfattention(x), last) and dyn.input_size == size
    assert torch.equal(dyn(x), static(x)) and dyn(x).shape == (4, cfg.dim)
    assert torch.equal(dyn.dense_tokens(x), static.dense_tokens(x))
    assert torch.equal(dyn.patch_embed(x), static.patch_embed(x))
    enc = dyn.image_encoder(x)
    assert enc.shape == (4, cfg.dim, gh, gw) and torch.equal(enc, static.image_encoder(x))
    a, b = dyn.get_intermediate_layers(x, 2, reshape=True, return_class_token=True), static.get_intermediate_layers(
        x, 2, reshape=True, return_class_token=True)
    assert a[0][0].shape == (4, cfg.dim, gh, gw)
    assert all(torch.equal(p, q) and torch.equal(c, d) for (p, c), (q, d) in zip(a, b))
    assert torch.equal(dyn.linear_probe_features(x, 2), static.linear_probe_features(x, 2))
    assert vdr.extract_dense(dyn, x).shape == (4, gh, gw, cfg.dim)
    # ... and goes back to the native size on its own: bitwise a model that never moved
    x0 = vo.make_images(cfg, 3, seed=23).cuda()
    assert torch.equal(dyn(x0), VitDescriptorModel(hc.vit_config(cfg), w)(x0)) and dyn.input_size == (56, 56)
    with pytest.raises(ValueError, match="images must be"):
        static(x0)  # without dynamic_size another shape is refused, as ever


# ---- 7. batch properties at a new size ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("p16_d128", (160, 96)), ("p14_d192", (84, 126))])
def test_batch_properties_at_a_new_size(name, size):
    """tests/model_gates.py's check_batch_properties: duplicate images give bitwise equal rows, a batch permutation permutes
    the rows, a row does not depend on the batch it travels in."""
    import vdr
    cfg = SMALL[name]
    e = _engine(cfg, vo.make_weights(cfg, seed=5, scale=0.05), size)
    B = 24
    x = _images(B, *size, seed=6)
    x[B - 1] = x[1]
    for dt in (torch.float32, torch.bfloat16):
        xd = x.cuda().to(dt)
        for mode in (vdr.OUT_CLS, vdr.OUT_DENSE):
            check_batch_properties(lambda t: e.forward(t, mode), xd)


# ---- 8. rectangular patch embedding, integer-exact ------------------------------------------------------------------
@pytest.mark.parametrize("p,img,size,D,dt", [(14, 56, (28, 518), 128, torch.float32), (14, 56, (518, 42), 128, torch.bfloat16),
                                             (16, 64, (48, 160), 192, torch.bfloat16), (16, 64, (160, 48), 192, torch.float32),
                                             (8, 32, (24, 72), 64, torch.bfloat16), (32, 64, (96, 160), 128, torch.bfloat16),
                                             (16, 64, (128, 128), 192, torch.bfloat16)])
def test_rectangular_patch_embed_integer_exact(p, img, size, D, dt):
    """In the manner of tests/test_ops_gpu.py's exact patch-embed tests, through a has_pos = 0 patch-embedding model and
    OUT_PATCH_EMBED: integer pixels and weights pin every (token, channel, ky, kx) -> operand mapping of the height x width
    im2col (LDS form with a ragged 37-patch row, direct form, fp32 and bf16 pixels) bit for bit; the last case is a square
    non-native size on the gathered path."""
    import vdr
    gen = torch.Generator().manual_seed(p * 1000 + size[0] + size[1])
    B = 3
    x = torch.randint(-3, 4, (B, 3, *size), generator=gen).float()
    Wt = torch.randint(-2, 3, (D, 3, p, p), generator=gen).float()
    b = torch.randint(-3, 4, (D,), generator=gen).float()
    ref = torch.nn.functional.conv2d(x, Wt, b, stride=p).flatten(2).transpose(1, 2)
    assert ref.abs().max() < 2 ** 24
    vc = vdr.VdrConfig(img, p, 3, D, D // 64, 0, 4 * D, pre_ln=False, has_cls=False, has_pos=False)
    e = vdr.Engine(vc)
    e.load_weights({"patch_embed.proj.weight": Wt, "patch_embed.proj.bias": b})
    e.set_input_size(*size)
    got = e.forward(x.cuda().to(dt), vdr.OUT_PATCH_EMBED)
    assert got.shape == ref.shape == (B, (size[0] // p) * (size[1] // p), D)
    assert torch.equal(got.cpu(), ref), f"patch embed {size} / {p} {dt}"


# ---- 9. full size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(224, 224), (448, 336)])
def test_vit_small14_native_518_at_other_sizes_full_depth(size):
    """The geometry of a real dinov2_vits14 checkpoint: pos_embed [1, 1370, 384] (518^2, seeded), all 12 blocks, batch 4."""
    import vdr
    cfg = vo.VitCfg(518, 14, 3, 384, 6, 12, 1536, act="gelu", layerscale=True)
    vc = vdr.ARCHS["dinov2_small14_518"]
    assert (vc.img, vc.patch, vc.dim, vc.heads, vc.layers, vc.mlp_hidden, vc.layerscale) == (518, 14, 384, 6, 12, 1536, True)
    w = vo.make_weights(cfg, seed=14)
    assert w["pos_embed"].shape == (1, 1370, 384)
    x = _images(4, *size, seed=15)
    ref = vo.forward_images(cfg, _weights_at(cfg, w, size), x)
    m = vdr.load_model("dinov2_small14_518", weights=w, dynamic_size=True)
    n = (size[0] // 14) * (size[1] // 14)
    dense = m.dense_tokens(x.cuda(), torch.float32)
    assert dense.shape == (4, n, 384) and m.input_size == size
    check_parity(dense, ref["dense"], f"ViT-S/14 (518 table) at {size} L=12 dense", gate_l2(12))
    check_parity(m(x.cuda()), ref["cls"], f"ViT-S/14 (518 table) at {size} L=12 cls", gate_l2(12))


def test_vit_base16_at_448_full_depth():
    import vdr
    cfg = vo.VitCfg(224, 16, 3, 768, 12, 12, 3072)
    w = vo.make_weights(cfg, seed=16)
    x = _images(8, 448, 448, seed=17)
    ref = vo.forward_images(cfg, _weights_at(cfg, w, (448, 448)), x)
    m = vdr.load_model("vit_base16_224", weights=w).set_input_size(448, 448)
    xd = x.cuda().to(torch.bfloat16)
    dense = m.dense_tokens(xd, torch.float32)
    assert dense.shape == (8, 784, 768)
    check_parity(dense, ref["dense"], "ViT-B/16 at 448^2 L=12 dense", gate_l2(12))
    check_parity(m(xd), ref["cls"], "ViT-B/16 at 448^2 L=12 cls", gate_l2(12))


# ---- 10. refusals on a live handle -------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import vdr
    sam = vdr.Engine(vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "layers": 2, "global_blocks": (1,)}))
    assert sam.lib.vdr_set_input_size(sam.h, 512, 512) == -7  # VDR_ERR_UNSUPPORTED
    assert b"SAM" in sam.lib.vdr_last_error(sam.h)
    tok = vdr.Engine(vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False,
                                   has_pos=False, input_ln=True, ln_eps=1e-5))
    assert tok.lib.vdr_set_input_size(tok.h, 64, 64) == -7
    cfg = SMALL["p16_d128"]
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    blank = vdr.Engine(hc.vit_config(cfg))
    assert blank.lib.vdr_set_input_size(blank.h, 128, 128) == -6  # VDR_ERR_INCOMPLETE: not finalised
    e = _engine(cfg, w)
    lib = e.lib
    for bad, word in (((72, 64), b"height"), ((64, 100), b"width")):
        assert lib.vdr_set_input_size(e.h, *bad) == -1  # VDR_ERR_INVALID
        assert word in lib.vdr_last_error(e.h) and b"multiple of patch" in lib.vdr_last_error(e.h)
    assert e.input_size == (64, 64)
    x0 = vo.make_images(cfg, 4, seed=4).cuda()
    want = e.forward(x0, vdr.OUT_CLS)  # (still the native geometry after the refusals)
    # a workspace sized for the old geometry: the existing error, not a fault
    old = e._workspace(4)
    old_bytes = old.numel()
    e.set_input_size(256, 256)
    need = C.c_size_t()
    assert lib.vdr_workspace_bytes(e.h, 4, 0, C.byref(need)) == 0 and need.value > old_bytes
    x = _images(4, 256, 256, seed=5).cuda()
    out = torch.empty((4, cfg.dim), dtype=torch.float32, device="cuda")
    rc = lib.vdr_forward(e.h, x.data_ptr(), 0, 4, out.data_ptr(), vdr.OUT_CLS, 0, old.data_ptr(), old_bytes,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == -5 and b"workspace too small" in lib.vdr_last_error(e.h)  # VDR_ERR_WORKSPACE
    assert e.forward(x, vdr.OUT_CLS).shape == (4, cfg.dim)  # the engine sizes its workspace again
    e.set_input_size(64, 64)
    assert torch.equal(e.forward(x0, vdr.OUT_CLS), want)


def test_forward_at_a_new_size_is_graph_capturable():
    """The hot-path promise holds at any size: all allocation happened in vdr_set_input_size, so the first forward after it
    can be captured into a HIP graph, and the replay reproduces an eager forward bit for bit."""
    import vdr
    cfg = SMALL["p16_d128"]
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    size = (96, 160)
    x = _images(5, *size, seed=2).cuda()
    e = _engine(cfg, w, size)
    out = torch.empty((5, cfg.dim), dtype=torch.float32, device="cuda")
    e._workspace(5)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            e.forward_into(x, out, vdr.OUT_CLS)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _engine(cfg, w, size).forward(x, vdr.OUT_CLS))
