"""GPU: dense descriptors at a patch stride below the patch side (vdr_set_patch_stride, csrc/patch_stride.hip).

The definition every model check uses is tests/stride_ref.py: F.conv2d(images, W, b, stride=s), pos_embed's patch rows
resampled in float64 to the (gh, gw) grid and rounded once, then the UNCHANGED oracle's assemble_tokens / encoder
(tests/test_patch_stride_cpu.py ties it to the oracle at s == p).  Model gates are the project's own
(tests/model_gates.py): min row cosine >= 0.999 and rel-L2 <= 4e-3 + 3e-3 sqrt(L) against the fp32 and the
bf16-emulating restatement.  The kernel itself is pinned bit for bit: integer data through vdr_op_patch_embed_strided, and
the shift property of the overlapping grid."""
import ctypes as C

import numpy as np
import pytest
import torch

import handle_configs as hc
import stride_ref as sr
from model_gates import check_batch_properties, check_parity, gate_l2, rel_l2
from ops_checks import bf
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _engine(cfg, w, size=None, stride=None, **kw):
    """An engine of cfg's weights, told `size` = (H, W) and `stride` when given (size first)."""
    e = hc.engine(cfg, w, **kw)
    if size is not None:
        e.set_input_size(*size)
    if stride is not None:
        e.set_patch_stride(stride)
    return e


def _images(batch, H, W, seed, chans=3):
    """[0, 1) pixels that bf16 holds exactly: fp32 and bf16 pixel buffers then carry the same values."""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    x = torch.from_numpy(rng.random(size=(batch, chans, H, W), dtype=np.float32))
    return x.to(torch.bfloat16).float()


def _registers(cfg, n, seed):
    z = np.random.Generator(np.random.PCG64([seed, 9001])).standard_normal(size=(1, n, cfg.dim), dtype=np.float32)
    return torch.from_numpy(0.02 * z)


SMALL = {  # tests/test_input_size_gpu.py's, plus register tokens and a CLIP-style input LayerNorm
    "p16_d128": (vo.VitCfg(64, 16, 3, 128, 2, 3, 512), 0),
    "p14_d192": (vo.VitCfg(56, 14, 3, 192, 3, 2, 768), 0),
    "dinov2_swiglu_ls": (vo.VitCfg(56, 14, 3, 128, 2, 2, 320 + 64, act="swiglu", layerscale=True), 0),
    "reg4_p16": (vo.VitCfg(64, 16, 3, 128, 2, 2, 512, layerscale=True), 4),
    "clip_input_ln": (vo.VitCfg(64, 16, 3, 128, 2, 2, 512, input_ln=True, ln_eps=1e-5), 0),
}


def _small(name, seed=3):
    cfg, nreg = SMALL[name]
    w = vo.make_weights(cfg, seed=seed, scale=0.05)
    reg = _registers(cfg, nreg, seed) if nreg else None
    wl = dict(w, register_tokens=reg) if nreg else w
    return cfg, w, wl, reg, dict(n_register=nreg) if nreg else {}


# ---- 1. integer-exact patch embedding through vdr_op_patch_embed_strided --------------------------------------------------
EXACT = [(16, 8, (48, 48)), (16, 4, (32, 80)), (16, 2, (32, 32)), (14, 7, (42, 70)), (14, 2, (28, 28)), (8, 4, (24, 40)),
         (32, 8, (64, 96)), (16, 8, (32, 16 + 8 * 40))]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p,s,size", EXACT, ids=[f"p{p}s{s}_{h}x{w}" for p, s, (h, w) in EXACT])
def test_strided_patch_embed_integer_exact(p, s, size, dt):
    """Small-integer pixels, weights, bias and pos: fp32 accumulation is exact, so the op must give F.conv2d(stride=s)
    (+ pos) bit for bit after its one rounding to bf16, and the col matrix it leaves IS the unfolded image: every
    (patch, channel, ky, kx) -> (row, column) mapping of the overlapping im2col, the zero K padding included (col is
    NaN-filled first).  C in {1, 3}, D in {64, 128}, batch 2; the last case has gw = 41: two tiles per patch row, the last
    one ragged."""
    from vdr import ops
    B = 2
    gh, gw = sr.grid(size, p, s)
    n = gh * gw
    for Cc in (1, 3):
        for D in (64, 128):
            gen = torch.Generator().manual_seed(p * 1000 + s * 100 + size[1] + Cc + D)
            x = torch.randint(-3, 4, (B, Cc, *size), generator=gen).float()
            Wt = torch.randint(-2, 3, (D, Cc, p, p), generator=gen).float()
            b = torch.randint(-3, 4, (D,), generator=gen).float()
            pos = torch.randint(-2, 3, (n + 1, D), generator=gen).float()
            ref = torch.nn.functional.conv2d(x, Wt, b, stride=s).flatten(2).transpose(1, 2)
            assert ref.shape == (B, n, D) and ref.abs().max() < 16384  # (exact in fp32; bf16 output: the same rounding)
            y, col = ops.patch_embed_strided(x.to(dt).cuda(), Wt.cuda(), b.cuda(), p, s, return_col=True)
            assert torch.equal(y.float().cpu(), bf(ref.reshape(B * n, D)).float()), (Cc, D)
            K = Cc * p * p
            unfold = torch.nn.functional.unfold(x, kernel_size=p, stride=s).transpose(1, 2).reshape(B * n, K)
            colc = col.float().cpu()
            assert torch.equal(colc[:, :K], unfold), (Cc, D)
            assert colc.shape[1] == (K + 63) // 64 * 64 and torch.equal(colc[:, K:], torch.zeros(B * n, colc.shape[1] - K))
            # with position rows, written behind one prefix row per image
            y2 = ops.patch_embed_strided(x.to(dt).cuda(), Wt.cuda(), b.cuda(), p, s, pos=pos.cuda(), row_stride=n + 1, row_offset=1)
            y2 = y2.float().cpu().reshape(B, n + 1, D)
            assert torch.equal(y2[:, 0], torch.zeros(B, D))
            assert torch.equal(y2[:, 1:], bf(ref + pos[1:]).float()), (Cc, D)


def test_strided_op_at_stride_p_and_plain_form():
    """stride == p is vdr_op_patch_embed's result (rectangular sizes included); stride 1 and a width that is no multiple of
    8 take the plain form of the kernel: the same exact answers"""
    from vdr import ops
    gen = torch.Generator().manual_seed(77)
    for p, s, size in ((16, 16, (32, 48)), (8, 1, (10, 13)), (8, 2, (12, 18)), (16, 1, (17, 20))):
        x = torch.randint(-3, 4, (2, 3, *size), generator=gen).float()
        Wt = torch.randint(-2, 3, (64, 3, p, p), generator=gen).float()
        b = torch.randint(-3, 4, (64,), generator=gen).float()
        ref = torch.nn.functional.conv2d(x, Wt, b, stride=s).flatten(2).transpose(1, 2).reshape(-1, 64)
        for dt in (torch.float32, torch.bfloat16):
            y = ops.patch_embed_strided(x.to(dt).cuda(), Wt.cuda(), b.cuda(), p, s)
            assert torch.equal(y.float().cpu(), bf(ref).float()), (p, s, size, dt)


# ---- 2. the shift property, bitwise ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,s,size", [(16, 8, (64, 96)), (16, 4, (48, 64)), (14, 7, (56, 84)), (32, 8, (96, 64)), (8, 2, (32, 40))])
def test_shift_property_is_bitwise(p, s, size):
    """fp32 images (both arms go through an im2col), no position rows (has_pos = 0: only the gather is compared), random
    pixels and weights: the PATCH_EMBED rows (py, px) of the stride-s grid with py, px multiples of p / s are bitwise the
    rows of the same handle at stride p on the same image, and those at offset (dy, dx) = (s, s) are bitwise the stride-p
    rows of the image cropped by that offset."""
    import vdr
    r, D, B = p // s, 128, 3
    gen = torch.Generator().manual_seed(p * 100 + s)
    x = torch.rand((B, 3, *size), generator=gen)
    e = vdr.Engine(vdr.VdrConfig(size[0], p, 3, D, D // 64, 0, 4 * D, pre_ln=False, has_cls=False, has_pos=False))
    e.load_weights({"patch_embed.proj.weight": torch.randn((D, 3, p, p), generator=gen) * 0.05,
                    "patch_embed.proj.bias": torch.randn((D,), generator=gen)})
    e.set_input_size(*size)
    e.set_patch_stride(s)
    gh, gw = e.grid
    assert (gh, gw) == sr.grid(size, p, s)
    fine = e.forward(x.cuda(), vdr.OUT_PATCH_EMBED).reshape(B, gh, gw, D)
    e.set_patch_stride(p)
    coarse = e.forward(x.cuda(), vdr.OUT_PATCH_EMBED).reshape(B, size[0] // p, size[1] // p, D)
    assert torch.equal(fine[:, ::r, ::r], coarse)
    e.set_input_size(size[0] - p, size[1] - p)
    xc = x[:, :, s:s + size[0] - p, s:s + size[1] - p].contiguous()
    shifted = e.forward(xc.cuda(), vdr.OUT_PATCH_EMBED).reshape(B, size[0] // p - 1, size[1] // p - 1, D)
    assert torch.equal(fine[:, 1::r, 1::r][:, :shifted.shape[1], :shifted.shape[2]], shifted)
    assert not torch.equal(fine[:, 1::r, 1::r][:, :coarse.shape[1] - 1, :coarse.shape[2] - 1], coarse[:, :-1, :-1])


# ---- 3. small models against the restatement ---------------------------------------------------------------------------------
def _cases(name):
    """(size, stride): p / 2 at the native size and at one rectangular size; p / 4 once"""
    cfg = SMALL[name][0]
    s, p = cfg.img, cfg.patch
    out = [((s, s), p // 2), ((s + p, s - p), p // 2)]
    if name == "p16_d128":
        out.append(((s, s + p), p // 4))
    return out


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_models_at_a_finer_stride(name):
    """CLS / DENSE / TOKENS / POOLED / PATCH_EMBED, fp32 and bf16 pixels, one engine moved from geometry to geometry;
    get_intermediate_layers / get_attention_maps come on the (gh, gw) grid and CLS attention rows sum to 1 over the new N."""
    import vdr
    from vdr.model import VitDescriptorModel
    cfg, w, wl, reg, kw = _small(name)
    e = _engine(cfg, wl, **kw)
    m = VitDescriptorModel(hc.vit_config(cfg, **kw), wl)
    g = gate_l2(cfg.layers)
    B, P = 4, 1 + (0 if reg is None else reg.shape[1])
    for k, (size, s) in enumerate(_cases(name)):
        x = _images(B, *size, seed=30 + k)
        ref = sr.forward_images(cfg, w, x, s, registers=reg)
        emu = sr.forward_images(cfg, w, x, s, emulate_bf16=True, registers=reg)
        gh, gw = ref["grid"]
        n = gh * gw
        e.set_patch_stride(s)  # (stride first, then the size: the other order is test 4's)
        e.set_input_size(*size)
        st = C.c_int()
        assert e.lib.vdr_get_patch_stride(e.h, C.byref(st)) == 0 and st.value == s == e.patch_stride
        assert e.grid == (gh, gw) and e.n_patches == n and e.n_tokens == n + P == ref["tokens"].shape[1]
        ref["pooled"], emu["pooled"] = ref["dense"].mean(1), emu["dense"].mean(1)
        for dt in (torch.float32, torch.bfloat16):
            xd = x.cuda().to(dt)
            tag = f"{name} {size[0]}x{size[1]} stride {s} {'bf16' if dt == torch.bfloat16 else 'fp32'} pixels"
            for mode, key in ((vdr.OUT_CLS, "cls"), (vdr.OUT_DENSE, "dense"), (vdr.OUT_TOKENS, "tokens")):
                check_parity(e.forward(xd, mode), ref[key], f"{tag} {key}", g, emu[key])
            pooled, = e.forward_layers(xd, [vdr.LayerOut(cfg.layers - 1, vdr.OUT_POOLED)])
            check_parity(pooled, ref["pooled"], f"{tag} pooled", g, emu["pooled"])
            check_parity(e.forward(xd, vdr.OUT_PATCH_EMBED), ref["patch_embed"], f"{tag} patch_embed", 4e-3, emu["patch_embed"])
        # the DINOv2-style outputs follow the grid
        m.set_input_size(*size).set_patch_stride(s)
        assert m.grid == (gh, gw) and m.patch_stride == s
        xd = x.cuda()
        (feat, cls), = m.get_intermediate_layers(xd, 1, reshape=True, return_class_token=True)
        assert feat.shape == (B, cfg.dim, gh, gw) and cls.shape == (B, cfg.dim)
        assert torch.equal(feat.permute(0, 2, 3, 1).reshape(B, n, cfg.dim).float(), e.forward(xd, vdr.OUT_DENSE))
        heat, = m.get_attention_maps(xd, layers=[cfg.layers - 1], cls_only=True, reshape=True)
        assert heat.shape == (B, cfg.heads, gh, gw)
        cls_rows = m.get_attention_maps(xd, cls_only=True)
        assert cls_rows.shape == (B, cfg.heads, n + P)
        assert torch.allclose(cls_rows.sum(-1), torch.ones(B, cfg.heads, device=cls_rows.device), atol=1e-5)
        assert torch.equal(heat, cls_rows[..., P:].reshape(B, cfg.heads, gh, gw))
        full = m.get_last_selfattention(xd)  # (q_rows up to the new N)
        assert full.shape == (B, cfg.heads, n + P, n + P) and torch.equal(full[:, :, 0], cls_rows)
        with pytest.raises(ValueError, match="q_rows"):
            m.engine.forward_attn_maps(xd, [vdr.AttnMap(0, q_rows=n + P + 1)])
        assert m.image_encoder(xd).shape == (B, cfg.dim, gh, gw) and m.patch_embed(xd).shape == (B, n, cfg.dim)
        assert vdr.extract_dense(m, xd).shape == (B, gh, gw, cfg.dim)


def test_dynamic_size_keeps_the_stride():
    import vdr
    from vdr.model import VitDescriptorModel
    cfg, w, wl, reg, kw = _small("p16_d128")
    dyn = VitDescriptorModel(hc.vit_config(cfg), w, dynamic_size=True).set_patch_stride(8)
    for size in ((64, 64), (96, 48), (64, 64)):
        x = _images(2, *size, seed=40).cuda()
        gh, gw = sr.grid(size, 16, 8)
        assert dyn.image_encoder(x).shape == (2, cfg.dim, gh, gw) and dyn.input_size == size and dyn.patch_stride == 8
        assert torch.equal(dyn.dense_tokens(x), _engine(cfg, w, size, 8).forward(x, vdr.OUT_DENSE, torch.bfloat16))


# ---- 4. there and back ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p16_d128", "dinov2_swiglu_ls", "reg4_p16"])
def test_there_and_back_is_bitwise_a_fresh_engine(name):
    """stride p -> p/2 -> p, interleaved with set_input_size in both orders: whatever the path, the features are bitwise
    those of a fresh engine taken straight to the final geometry (bf16 pixels at the default stride: the im2col-free
    gather is restored, too)."""
    import vdr
    cfg, w, wl, reg, kw = _small(name)
    p, s0 = cfg.patch, cfg.img
    other = (s0 + p, s0 - p)
    x0 = vo.make_images(cfg, 5, seed=4).cuda()
    xo = _images(3, *other, seed=5).cuda()
    modes = (vdr.OUT_CLS, vdr.OUT_DENSE)

    def same(e, x, size, stride):
        fresh = _engine(cfg, wl, size, stride, **kw)
        for dt in (torch.float32, torch.bfloat16):
            for m in modes:
                assert torch.equal(e.forward(x.to(dt), m), fresh.forward(x.to(dt), m)), (name, size, stride, dt, m)

    e = _engine(cfg, wl, **kw)
    assert e.patch_stride == p
    e.set_patch_stride(p // 2)
    assert e.forward(x0, vdr.OUT_DENSE).shape[1] == (2 * s0 // p - 1) ** 2
    e.set_patch_stride(p)
    same(e, x0, None, None)                       # p -> p/2 -> p at the native size: an engine that never moved
    e.set_patch_stride(p // 2)
    e.set_input_size(*other)
    same(e, xo, other, p // 2)                    # stride, then size
    e.set_patch_stride(p)
    same(e, xo, other, None)                      # back to p at the other size: set_input_size alone
    e.set_input_size(s0, s0)
    same(e, x0, None, None)
    e.set_input_size(*other)
    e.set_patch_stride(p // 2)
    e.set_input_size(s0, s0)
    same(e, x0, None, p // 2)                     # size, stride, size: the stride stays in force
    e.set_patch_stride(p)
    same(e, x0, None, None)


# ---- 5. batch properties at stride p / 2 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("p16_d128", (96, 64)), ("p14_d192", (56, 84))])
def test_batch_properties_at_a_finer_stride(name, size):
    """duplicate images give bitwise equal rows, a batch permutation permutes the rows, a row does not depend on the batch
    it travels in"""
    import vdr
    cfg, w, wl, reg, kw = _small(name, seed=5)
    e = _engine(cfg, wl, size, cfg.patch // 2)
    B = 24
    x = _images(B, *size, seed=6)
    x[B - 1] = x[1]
    for dt in (torch.float32, torch.bfloat16):
        xd = x.cuda().to(dt)
        for mode in (vdr.OUT_CLS, vdr.OUT_DENSE):
            check_batch_properties(lambda t: e.forward(t, mode), xd)


# ---- 6. token counts across the attention launcher's classes -----------------------------------------------------------------------
@pytest.mark.parametrize("size,s,N", [((80, 64), 8, 64), ((48, 112), 8, 66), ((32, 112), 4, 126), ((64, 160), 8, 134),
                                      ((112, 144), 8, 222), ((128, 128), 8, 226), ((64, 336), 8, 288), ((144, 144), 8, 290)])
def test_token_counts_across_the_attention_classes(size, s, N):
    """<= 64, <= 128, <= 224, <= 288, > 288 tokens (tests/test_input_size_gpu.py's boundaries), reached from both sides by
    the odd grids of a finer stride: one small p = 16 model (native 96^2)."""
    import vdr
    cfg = vo.VitCfg(96, 16, 3, 128, 2, 2, 512)
    w = vo.make_weights(cfg, seed=8, scale=0.05)
    x = _images(3, *size, seed=9)
    ref = sr.forward_images(cfg, w, x, s)
    emu = sr.forward_images(cfg, w, x, s, emulate_bf16=True)
    assert ref["tokens"].shape[1] == N
    e = _engine(cfg, w, size, s)
    assert e.n_tokens == N
    g = gate_l2(cfg.layers)
    for dt in (torch.float32, torch.bfloat16):
        for mode, key in ((vdr.OUT_CLS, "cls"), (vdr.OUT_TOKENS, "tokens")):
            check_parity(e.forward(x.cuda().to(dt), mode), ref[key], f"N={N} {size} stride {s} {dt} {key}", g, emu[key])


# ---- 7. refusals on a live handle, workspace ------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle_and_workspace():
    import vdr
    sam = vdr.Engine(vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "layers": 2, "global_blocks": (1,)}))
    assert sam.lib.vdr_set_patch_stride(sam.h, 8) == -7  # VDR_ERR_UNSUPPORTED
    assert b"SAM" in sam.lib.vdr_last_error(sam.h)
    tok = vdr.Engine(vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False,
                                   has_pos=False, input_ln=True, ln_eps=1e-5))
    assert tok.lib.vdr_set_patch_stride(tok.h, 8) == -7 and b"token model" in tok.lib.vdr_last_error(tok.h)
    post = vdr.Engine(vdr.VdrConfig(img=64, patch=16, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False))
    assert post.lib.vdr_set_patch_stride(post.h, 8) == -7 and b"pre-LN" in post.lib.vdr_last_error(post.h)
    rope = vdr.Engine(vdr.VdrConfig(img=64, patch=16, dim=128, heads=2, layers=1, mlp_hidden=256, has_pos=False, n_register=4,
                                    rope=True))
    assert rope.lib.vdr_set_patch_stride(rope.h, 8) == -7 and b"rope" in rope.lib.vdr_last_error(rope.h)
    with pytest.raises(ValueError, match="RoPE"):
        rope.set_patch_stride(8)
    # the argument refusals come before the model's (order of the header): a stride that does not divide patch is INVALID
    # on the SAM handle too
    for bad in (32, 5):
        assert sam.lib.vdr_set_patch_stride(sam.h, bad) == -1 and b"divide patch 16" in sam.lib.vdr_last_error(sam.h)
    cfg, w, wl, reg, kw = _small("p16_d128")
    blank = vdr.Engine(hc.vit_config(cfg))
    assert blank.lib.vdr_set_patch_stride(blank.h, 8) == -6  # VDR_ERR_INCOMPLETE: not finalised
    st = C.c_int()
    assert blank.lib.vdr_get_patch_stride(blank.h, C.byref(st)) == 0 and st.value == 16  # patch until the first set
    e = _engine(cfg, w)
    lib = e.lib
    B = 16  # (16 x 17 -> 16 x 50 token rows: past a 256-row step of the workspace's row padding)
    x0 = vo.make_images(cfg, B, seed=4).cuda()
    want = e.forward(x0, vdr.OUT_CLS)
    # a workspace sized at stride p: the existing error at stride p / 2, not a fault
    old = e._workspace(B)
    old_bytes = old.numel()
    e.set_patch_stride(8)
    need = C.c_size_t()
    assert lib.vdr_workspace_bytes(e.h, B, 0, C.byref(need)) == 0 and need.value > old_bytes
    out = torch.empty((B, cfg.dim), dtype=torch.float32, device="cuda")
    rc = lib.vdr_forward(e.h, x0.data_ptr(), 0, B, out.data_ptr(), vdr.OUT_CLS, 0, old.data_ptr(), old_bytes,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == -5 and b"workspace too small" in lib.vdr_last_error(e.h)  # VDR_ERR_WORKSPACE
    assert e.forward(x0, vdr.OUT_CLS).shape == (B, cfg.dim)  # the engine sizes its workspace again
    assert e._workspace(B).numel() == need.value
    e.set_patch_stride(16)
    assert torch.equal(e.forward(x0, vdr.OUT_CLS), want)


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------------
def test_forward_at_a_finer_stride_is_graph_capturable():
    """The hot-path promise holds at any stride: all allocation happened in vdr_set_patch_stride, so the first forward after
    it can be captured into a HIP graph (one linear stream), and the replay reproduces an eager forward bit for bit."""
    import vdr
    cfg, w, wl, reg, kw = _small("p16_d128")
    size = (96, 64)
    x = _images(5, *size, seed=2).cuda()
    e = _engine(cfg, w, size, 8)
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
    assert torch.equal(out, _engine(cfg, w, size, 8).forward(x, vdr.OUT_CLS))


# ---- 9. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface(monkeypatch):
    """load_model(..., stride=8) on a seeded ViT-B/16-shaped tiny config; get_dense_descriptor gives (gh, gw, D) float32;
    generate_features crops the (gh, gw) maps with the host box maths applied to that grid."""
    import vdr
    from vdr import pipeline
    vc = vdr.VdrConfig(img=96, patch=16, dim=128, heads=2, layers=2, mlp_hidden=512)
    cfg = vo.VitCfg(96, 16, 3, 128, 2, 2, 512)
    w = vo.make_weights(cfg, seed=11, scale=0.05)
    monkeypatch.setitem(vdr.ARCHS, "tiny_b16", vc)
    model = vdr.load_model("tiny_b16", weights=w, stride=8)
    assert model.patch_stride == 8 and model.grid == (11, 11)
    x = _images(1, 96, 96, seed=12)
    d = vdr.get_dense_descriptor(model, x[0])
    assert d.shape == (11, 11, 128) and d.dtype == np.float32
    want = sr.forward_images(cfg, w, x, 8)["patch_embed"][0].reshape(11, 11, 128)
    assert rel_l2(torch.from_numpy(d), want) <= 4e-3
    rng = np.random.default_rng(8)
    H, W, S = 72, 80, 2
    img = rng.random((H, W, S, 3)).astype(np.float32)
    mask = np.zeros((H, W, S), dtype=bool)
    mask[30:41, 36:50, :] = True
    feats, masks = pipeline.generate_features(model, img, mask)
    assert len(feats) == S and len(masks) == S
    # the host box maths of the pipeline, on the 11 x 11 grid
    bigger = mask.sum(-1) > 0
    xmin, ymin, xmax, ymax = pipeline.extract_coords(bigger, margin=2)
    cs = max(xmax - xmin, ymax - ymin) * 2
    xm, ym = int(xmin + (xmax - xmin) / 2), int(ymin + (ymax - ymin) / 2)
    y0, y1, x0, x1 = pipeline.crop_box((H, W), xm - cs, ym - cs, xm + cs, ym + cs)
    big_c = bigger[y0:y1, x0:x1]
    rb = pipeline.roi_box((11, 11), big_c)
    fy0, fy1, fx0, fx1 = pipeline.crop_box((11, 11), *rb)
    assert (fy1 - fy0, fx1 - fx0) != pipeline.crop_box((6, 6), *pipeline.roi_box((6, 6), big_c))[1::2]  # (not the stride-p box)
    from vdr import prep
    xs = prep.prepare_slices(torch.from_numpy(img[y0:y1, x0:x1]), side=96, out_dtype=torch.bfloat16, device=model.device)
    maps = model.engine.forward(xs, vdr.OUT_PATCH_EMBED, torch.float32).reshape(S, 11, 11, 128)
    for i in range(S):
        assert feats[i].shape == (fy1 - fy0, fx1 - fx0, 128) and feats[i].dtype == np.float32
        assert np.array_equal(feats[i], maps[i, fy0:fy1, fx0:fx1].cpu().numpy())
        assert np.array_equal(masks[i], pipeline.crop_image(mask[y0:y1, x0:x1, i] > 0, *pipeline.roi_box(big_c.shape, big_c)))
