"""GPU: vdr_forward_layers -- features from inside the encoder, several per forward.

Layer i of an L-block model must be, bit for bit, the output of the same weights truncated to i + 1 blocks (it is the same
final-LayerNorm launch on the same stream).  The raw stream (norm = 0) normalised by the LayerNorm op must give the
normalised output bit for bit.  The mean-pooled output is gated against the float64 mean of the same call's dense output;
the gate is tight enough to reject pooling that counts the CLS row, drops a patch row or divides by n + 1 (each an
O(1/n) error), and the test shows that it does."""
import ctypes as C

import pytest
import torch

import handle_configs as hc
from model_gates import check_parity, gate_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

MODES = ("cls", "dense", "tokens")


def _engine(cfg, w, layers=None, **kw):
    """An engine of cfg's weights truncated to `layers` blocks (load_weights is strict: only blocks 0 .. layers-1)."""
    L = cfg.layers if layers is None else layers
    return hc.engine(cfg, hc.first_blocks(w, L), layers=L, **kw)


def _mode(name):
    import vdr
    return {"cls": vdr.OUT_CLS, "dense": vdr.OUT_DENSE, "tokens": vdr.OUT_TOKENS, "pooled": vdr.OUT_POOLED}[name]


VIT4 = vo.VitCfg(64, 16, 3, 128, 2, 4, 512)
DINO384 = vo.VitCfg(56, 14, 3, 384, 6, 3, 1024, act="swiglu", layerscale=True)
DINO192 = vo.VitCfg(56, 14, 3, 192, 3, 3, 512, act="swiglu", layerscale=True)
PATHS = {
    "fold": (dict(), 3),
    "no_ln_fold": (dict(ln_fold=False), 3),
    "resid_fp32": (dict(resid_fp32=True), 3),
    "fp8": (dict(fp8=1), 3),
    "fp8_cls_bf16": (dict(fp8=1, fp8_cls_bf16=True), 3),
    "mb3_streams2": (dict(micro_batch=3, streams=2), 7),
}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("model", ["vit4", "dino384", "dino192"])
def test_truncation_identity_bitwise(model, path):
    """Every layer, every mode (CLS / DENSE / TOKENS), both dtypes, from ONE forward_layers call of the full model, against
    vdr_forward of the model truncated to layer + 1 blocks."""
    import vdr
    cfg = {"vit4": VIT4, "dino384": DINO384, "dino192": DINO192}[model]
    kw, B = PATHS[path]
    w = vo.make_weights(cfg, seed=31, scale=0.05)
    x = vo.make_images(cfg, B, seed=32).cuda()
    full = _engine(cfg, w, **kw)
    specs = [vdr.LayerOut(i, _mode(m), dt) for i in range(cfg.layers) for m in MODES for dt in (torch.float32, torch.bfloat16)]
    got = full.forward_layers(x, specs)
    for i in range(cfg.layers):
        trunc = _engine(cfg, w, layers=i + 1, **kw)
        for sp, g in zip(specs, got):
            if sp.layer != i:
                continue
            want = trunc.forward(x, sp.mode, sp.dtype)
            assert torch.isfinite(want.float()).all()
            assert torch.equal(g, want), f"{model} {path}: layer {i} mode {sp.mode} {sp.dtype}"
    # the layers differ from each other (the comparison is not vacuous)
    assert not torch.equal(got[0], got[6])


def test_last_layer_equals_forward_at_full_size():
    """ViT-B/16, batch 256: layer 11 equals vdr_forward bit for bit -- CLS alone (the last block on its CLS rows only)
    and DENSE (the full last block), each with and without an earlier layer requested in the same call."""
    import vdr
    cfg = vo.VitCfg()
    w = vo.make_weights(cfg, seed=41, scale=0.02)
    x = vo.make_images(cfg, 256, seed=42).cuda().to(torch.bfloat16)
    e = _engine(cfg, w)
    ref_cls = e.forward(x, vdr.OUT_CLS)
    ref_dense = e.forward(x, vdr.OUT_DENSE)
    (cls,) = e.forward_layers(x, [vdr.LayerOut(11, vdr.OUT_CLS)])
    assert torch.equal(cls, ref_cls)
    (dense,) = e.forward_layers(x, [vdr.LayerOut(11, vdr.OUT_DENSE)])
    assert torch.equal(dense, ref_dense)
    cls5, cls2, dense2 = e.forward_layers(x, [vdr.LayerOut(5, vdr.OUT_CLS), vdr.LayerOut(11, vdr.OUT_CLS),
                                              vdr.LayerOut(11, vdr.OUT_DENSE)])
    assert torch.equal(cls2, ref_cls) and torch.equal(dense2, ref_dense)
    assert not torch.equal(cls5, ref_cls)


@pytest.mark.parametrize("resid_fp32", [False, True])
def test_raw_stream_normalised_by_the_op_equals_the_normalised_output(resid_fp32):
    import vdr
    from vdr import ops
    cfg = DINO384
    w = vo.make_weights(cfg, seed=51, scale=0.05)
    x = vo.make_images(cfg, 5, seed=52).cuda()
    e = _engine(cfg, w, resid_fp32=resid_fp32)
    src = torch.float32 if resid_fp32 else torch.bfloat16  # the stream's own dtype: the raw copy is exact
    gam, bet = w["norm.weight"].cuda(), w["norm.bias"].cuda()
    for i in range(cfg.layers):
        raw_t, raw_c, nt, nc, ntb = e.forward_layers(x, [
            vdr.LayerOut(i, vdr.OUT_TOKENS, src, norm=False), vdr.LayerOut(i, vdr.OUT_CLS, src, norm=False),
            vdr.LayerOut(i, vdr.OUT_TOKENS, torch.float32), vdr.LayerOut(i, vdr.OUT_CLS, torch.float32),
            vdr.LayerOut(i, vdr.OUT_TOKENS, torch.bfloat16)])
        assert torch.equal(raw_c, raw_t[:, 0])
        assert torch.equal(ops.layernorm(raw_t, gam, bet, cfg.ln_eps, out_dtype=torch.float32), nt), f"layer {i}"
        assert torch.equal(ops.layernorm(raw_t, gam, bet, cfg.ln_eps, out_dtype=torch.bfloat16), ntb), f"layer {i}"
        assert torch.equal(nc, nt[:, 0])
        # a raw bf16 copy of the fp32 stream is its one rounding
        (rb,) = e.forward_layers(x, [vdr.LayerOut(i, vdr.OUT_DENSE, torch.bfloat16, norm=False)])
        assert torch.equal(rb, raw_t[:, 1:].to(torch.bfloat16))


def _pool_check(e, x, layer, n, what):
    """Pooled (fp32 and bf16, normalised and raw) against the float64 mean of the same call's dense output."""
    import vdr
    outs = e.forward_layers(x, [vdr.LayerOut(layer, vdr.OUT_POOLED), vdr.LayerOut(layer, vdr.OUT_POOLED, torch.bfloat16),
                                vdr.LayerOut(layer, vdr.OUT_TOKENS),
                                vdr.LayerOut(layer, vdr.OUT_POOLED, norm=False), vdr.LayerOut(layer, vdr.OUT_TOKENS, norm=False)])
    pooled, pooled_bf, tokens, raw_pooled, raw_tokens = [t.cpu() for t in outs]
    assert tokens.shape[1] == n + 1
    assert torch.equal(pooled_bf, pooled.to(torch.bfloat16)), f"{what}: bf16 output is not bf16(fp32 output)"
    for got, tok, kind in ((pooled, tokens, "norm"), (raw_pooled, raw_tokens, "raw")):
        dense = tok[:, 1:].double()
        ref = dense.mean(dim=1)
        gate = 1e-5 * dense.abs().max().item()
        err = (got.double() - ref).abs().max().item()
        print(f"{what} {kind}: n {n} max|err| {err:.3e} gate {gate:.3e}")
        assert err <= gate, f"{what} {kind}: pooled max|err| {err} > {gate}"
        if kind == "raw":
            continue
        # the gate rejects the O(1/n) bugs: counting the CLS row, dropping a row, dividing by n + 1 (the final norm's
        # bias is shifted by 1 in these tests, so that every column mean is O(1))
        wrong = {"with CLS row": tok.double().mean(dim=1), "last row dropped": dense[:, :-1].mean(dim=1),
                 "divided by n + 1": dense.sum(dim=1) / (n + 1)}
        for bug, val in wrong.items():
            assert (val - ref).abs().max().item() > 4 * gate, f"{what} {kind}: the gate would not catch '{bug}'"
    return pooled


@pytest.mark.parametrize("img,patch,dim,heads,mlp", [
    (64, 16, 128, 2, 512),     # n = 16: one chunk
    (98, 14, 192, 3, 512),     # n = 49: one ragged chunk
    (224, 16, 128, 2, 512),    # n = 196: 3 chunks + a ragged one of 4 rows
    (224, 14, 384, 6, 1024),   # n = 256 (N = 257): 4 whole chunks
])
def test_pooled_against_float64_mean(img, patch, dim, heads, mlp):
    cfg = vo.VitCfg(img, patch, 3, dim, heads, 2, mlp)
    w = vo.make_weights(cfg, seed=61, scale=0.05)
    w["norm.bias"] = w["norm.bias"] + 1.0  # column means well away from 0, so that a 1/(n+1) scale shows
    x = vo.make_images(cfg, 3, seed=62).cuda()
    e = _engine(cfg, w)
    for layer in (0, 1):
        _pool_check(e, x, layer, cfg.n_patches, f"{img}/{patch} D {dim} layer {layer}")


def test_pooled_dinov2_small_896():
    """DINOv2-S/14 at 896^2: n = 4096 patch rows (64 chunks), D = 384, LayerScale + SwiGLU, bf16 images."""
    cfg = vo.VitCfg(896, 14, 3, 384, 6, 1, 1536, act="swiglu", layerscale=True)
    w = vo.make_weights(cfg, seed=71, scale=0.05)
    w["norm.bias"] = w["norm.bias"] + 1.0
    x = vo.make_images(cfg, 2, seed=72).cuda().to(torch.bfloat16)
    _pool_check(_engine(cfg, w), x, 0, 4096, "dinov2_s14@896")


def test_pooled_is_deterministic_and_batch_invariant():
    import vdr
    cfg = vo.VitCfg(224, 16, 3, 128, 2, 2, 512)
    w = vo.make_weights(cfg, seed=81, scale=0.05)
    x = vo.make_images(cfg, 7, seed=82).cuda()
    spec = [vdr.LayerOut(1, vdr.OUT_POOLED), vdr.LayerOut(0, vdr.OUT_POOLED, norm=False), vdr.LayerOut(1, vdr.OUT_DENSE)]
    mb = _engine(cfg, w, micro_batch=3, streams=2)
    a = mb.forward_layers(x, spec)
    b = mb.forward_layers(x, spec)
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two runs differ"
    one = _engine(cfg, w)
    for i in (0, 3, 6):
        alone = one.forward_layers(x[i:i + 1], spec)
        assert torch.equal(alone[2][0], a[2][i]), f"image {i}: the stream itself depends on the batch"
        assert torch.equal(alone[0][0], a[0][i]), f"image {i}: pooled differs alone vs in the batch"
        assert torch.equal(alone[1][0], a[1][i]), f"image {i}: raw pooled differs alone vs in the batch"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_column_slices_of_one_matrix(dtype):
    """CLS of layers L-4 .. L-1 and the pooled vector of L-1 in one NaN-filled [B, 5D + 7] buffer (ld = 5D + 7: rows
    not vector-aligned): each slice equals the same output written alone, the 7 padding columns stay NaN."""
    import vdr
    cfg = vo.VitCfg(64, 16, 3, 128, 2, 5, 512)
    w = vo.make_weights(cfg, seed=91, scale=0.05)
    x = vo.make_images(cfg, 6, seed=92).cuda()
    e = _engine(cfg, w, micro_batch=4, streams=2)
    D, B, ld = cfg.dim, 6, 5 * cfg.dim + 7
    buf = torch.full((B, ld), float("nan"), dtype=dtype, device="cuda")
    specs = [vdr.LayerOut(cfg.layers - 4 + k, vdr.OUT_CLS, out=buf[:, k * D:(k + 1) * D]) for k in range(4)]
    specs.append(vdr.LayerOut(cfg.layers - 1, vdr.OUT_POOLED, out=buf[:, 4 * D:5 * D]))
    e.forward_layers(x, specs)
    for k, sp in enumerate(specs):
        (alone,) = e.forward_layers(x, [vdr.LayerOut(sp.layer, sp.mode, dtype)])
        assert torch.equal(buf[:, k * D:(k + 1) * D], alone), f"slice {k}"
    assert torch.isnan(buf[:, 5 * D:].float()).all(), "padding columns were written"


def test_refusals_with_a_real_handle_leave_the_output_untouched():
    import vdr
    from vdr import _lib
    lib = _lib.load()
    cfg = vo.VitCfg(64, 16, 3, 128, 2, 2, 512)
    e = _engine(cfg, vo.make_weights(cfg, seed=1, scale=0.05))
    x = vo.make_images(cfg, 2, seed=2).cuda()
    out = torch.full((2, 4 * 128), 7.0, device="cuda")
    ws = e._workspace(2)

    def call(eng, **kw):
        o = _lib.vdr_layer_out(layer=0, out_mode=vdr.OUT_CLS, out_dtype=_lib.VDR_F32, norm=1, ld=0, out=out.data_ptr())
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.vdr_forward_layers(eng.h, x.data_ptr(), 0, 2, C.byref(o), 1, ws.data_ptr(), ws.numel(), None)
    for kw in (dict(layer=2), dict(layer=-1), dict(ld=100), dict(ld=1)):
        assert call(e, **kw) == -1, kw
    nocls = vdr.Engine(hc.vit_config(vo.VitCfg(64, 16, 3, 128, 2, 2, 512, has_cls=False)))
    assert call(nocls) == -1 and b"cls" in lib.vdr_last_error(nocls.h)
    for vc in (vdr.ARCHS["medsam"], vdr.VdrConfig(64, 16, 3, 128, 2, 0, 512),
               vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=128, heads=2, layers=2, mlp_hidden=512, pre_ln=False, has_pos=False),
               vdr.VdrConfig(64, 16, 3, 128, 2, 2, 512, pre_ln=False)):
        assert call(vdr.Engine(vc)) == -7, vc  # VDR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call(e, ld=4 * 128) == 0
    torch.cuda.synchronize()
    assert not (out[:, :128] == 7.0).all() and (out[:, 128:] == 7.0).all()


def test_python_api_matches_dinov2_semantics_against_the_oracle():
    import dataclasses

    import vdr
    cfg = vo.VitCfg(112, 14, 3, 192, 3, 5, 512, act="swiglu", layerscale=True)
    w = vo.make_weights(cfg, seed=101, scale=0.05)
    x = vo.make_images(cfg, 3, seed=102)
    model = vdr.VitDescriptorModel(hc.vit_config(cfg), w)
    ref = {i: vo.forward_images(dataclasses.replace(cfg, layers=i + 1), w, x) for i in range(cfg.layers)}
    g, D, n = cfg.img // cfg.patch, cfg.dim, cfg.n_patches
    # n as an int: the last n blocks, patch tokens only
    outs = model.get_intermediate_layers(x.cuda(), 2)
    assert isinstance(outs, tuple) and len(outs) == 2
    for t, i in zip(outs, (3, 4)):
        assert t.shape == (3, n, D) and t.dtype == torch.float32
        check_parity(t, ref[i]["dense"], f"get_intermediate_layers block {i}", gate_l2(i + 1))
    # a list of blocks, reshaped, with class tokens: ((patch [B, D, h, w], cls [B, D]), ...) in block order
    outs = model.get_intermediate_layers(x.cuda(), [3, 0], reshape=True, return_class_token=True)
    assert len(outs) == 2 and all(len(p) == 2 for p in outs)
    for (patch, cls), i in zip(outs, (0, 3)):
        assert patch.shape == (3, D, g, g) and cls.shape == (3, D)
        assert patch.is_contiguous()  # DINOv2: reshape(B, h, w, D).permute(0, 3, 1, 2).contiguous()
        check_parity(patch.permute(0, 2, 3, 1).reshape(3, n, D), ref[i]["dense"], f"reshaped block {i}", gate_l2(i + 1))
        check_parity(cls, ref[i]["cls"], f"class token block {i}", gate_l2(i + 1))
    # norm=False: the raw stream (no final norm), against the oracle's stream before its final LayerNorm
    (raw,) = model.get_intermediate_layers(x.cuda(), [2], norm=False)
    normed = model.get_intermediate_layers(x.cuda(), [2])[0]
    assert not torch.allclose(raw, normed)
    with pytest.raises(ValueError):
        model.get_intermediate_layers(x.cuda(), [5])
    # create_linear_input(get_intermediate_layers(x, 4, return_class_token=True), 4, avgpool=True)
    feats = model.linear_probe_features(x.cuda(), n_last_blocks=4, avgpool=True)
    assert feats.shape == (3, 5 * D) and feats.dtype == torch.float32
    want = torch.cat([ref[i]["cls"] for i in (1, 2, 3, 4)] + [ref[4]["dense"].mean(dim=1)], dim=-1)
    for k in range(5):
        check_parity(feats[:, k * D:(k + 1) * D], want[:, k * D:(k + 1) * D], f"linear probe slice {k}", gate_l2(cfg.layers))
    # ... and it is exactly what the DINOv2 recipe computes from this model's own intermediate layers
    li = model.get_intermediate_layers(x.cuda(), 4, return_class_token=True)
    recipe = torch.cat([c for _, c in li] + [li[-1][0].double().mean(dim=1).float()], dim=-1)
    assert torch.equal(feats[:, :4 * D], recipe[:, :4 * D])
    assert (feats[:, 4 * D:] - recipe[:, 4 * D:]).abs().max() <= 1e-5 * li[-1][0].abs().max()
    assert model.linear_probe_features(x.cuda(), 2, avgpool=False).shape == (3, 2 * D)
