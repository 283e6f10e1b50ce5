"""GPU: SAM's box-prompt encoder and mask decoder -- the three kernels of csrc/mask_decoder.hip at op level (designed inputs
bit for bit, random inputs inside the fp32 bounds tests/sam_decoder_ref.py derives, problem independence, operands read in
place as column slices, output rows bounded by canaries), the whole decode against the transformers.SamModel goldens, the
whole path image -> mask, the bitwise properties of the public calls, and pipeline.segment_volume feeding generate_features.

Gates of the decode (tests/golden/README_sam_decoder.md): measured on the CPU by the golden generator as the difference of
the restatement's bf16-rounding mode from the golden, stored in the golden file, and doubled here (the device's fp32 sums
associate differently).  Nothing is derived from the device's output."""
import contextlib
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
import memguard as mg
import sam_decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bf(t):
    return t.to(torch.bfloat16).to(DEV)


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16)


# ---- cross attention -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tq,tk,dh,P", [(100, 8, 16, 3), (7, 8, 32, 2), (7, 64, 16, 3), (7, 4096, 16, 2), (16, 64, 32, 2), (5, 4096, 32, 1)])
def test_cross_attention_equal_keys_is_the_mean_of_the_values_bit_for_bit(tq, tk, dh, P):
    """all keys of a problem equal -> every p is exactly 1 (1 / tk after the one division); values are small integers, so
    sum p v is exact in any order and the output is bf16(fp32(sum v) / fp32(tk)); tk = 8 the few-keys regime, 64 (two of the
    four waves see no key) and 4096 the few-queries regime"""
    from vdr import ops
    H = 8
    HD = H * dh
    q = _rand((P * tq, HD), 1)
    krow = _rand((P, 1, HD), 2)
    k = krow.expand(P, tk, HD).reshape(P * tk, HD).contiguous()
    v = torch.randint(-8, 9, (P * tk, HD), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    out = ops.cross_attention(q.to(DEV), k.to(DEV), v.to(DEV), P, tq, tk, H, dh)
    torch.cuda.synchronize()
    mean = (v.double().reshape(P, tk, HD).sum(1).float() / float(tk)).to(torch.bfloat16)     # one fp32 division, one rounding
    want = mean[:, None].expand(P, tq, HD).reshape(P * tq, HD)
    assert torch.equal(out.cpu().view(torch.int16), want.contiguous().view(torch.int16))


SHAPES = [(7, 100, 16, 3), (7, 4096, 16, 2), (100, 7, 16, 3), (4096, 7, 16, 1), (7, 7, 32, 5), (1, 1, 16, 1), (16, 16, 32, 2)]


@pytest.mark.parametrize("tq,tk,dh,P", SHAPES)
def test_cross_attention_stays_inside_the_fp32_bound(tq, tk, dh, P):
    from vdr import ops
    H = 8
    HD = H * dh
    q, k, v = _rand((P * tq, HD), 11), _rand((P * tk, HD), 12), _rand((P * tk, HD), 13)
    g = torch.Generator().manual_seed(14)
    qa, ka = torch.randn((tq, HD), generator=g), torch.randn((tk, HD), generator=g)
    for q_add, k_add in ((None, None), (qa, ka)):
        out = ops.cross_attention(q.to(DEV), k.to(DEV), v.to(DEV), P, tq, tk, H, dh,
                                  q_add=None if q_add is None else q_add.to(DEV), k_add=None if k_add is None else k_add.to(DEV))
        torch.cuda.synchronize()
        exact, bound = R.cross_attention_ref(q, k, v, P, tq, tk, H, dh, q_add, k_add)
        err = (out.double().cpu() - R.bf16(exact)).abs()
        print(f"cross_attention {tq}x{tk} dh {dh} P {P} tables {q_add is not None}: max |out - bf16(exact)| {float(err.max()):.3e}, "
              f"max fp32 bound {float(bound.max()):.3e}, {int((err > 0).sum())} of {err.numel()} outputs off bf16(exact)")
        assert R.within_bf16_of(out, exact, bound)


@pytest.mark.parametrize("tq,tk,dh", [(7, 100, 16), (100, 7, 16), (7, 7, 32), (7, 300, 32)])
def test_cross_attention_problem_bits_do_not_depend_on_the_call(tq, tk, dh):
    from vdr import ops
    H, P = 8, 5
    HD = H * dh
    q, k, v = _bf(_rand((P * tq, HD), 21)), _bf(_rand((P * tk, HD), 22)), _bf(_rand((P * tk, HD), 23))
    ka = torch.randn((tk, HD), generator=torch.Generator().manual_seed(24)).to(DEV)
    full = ops.cross_attention(q, k, v, P, tq, tk, H, dh, k_add=ka)
    again = ops.cross_attention(q, k, v, P, tq, tk, H, dh, k_add=ka)
    assert torch.equal(full, again)
    for p in range(P):
        one = ops.cross_attention(q[p * tq:(p + 1) * tq], k[p * tk:(p + 1) * tk], v[p * tk:(p + 1) * tk], 1, tq, tk, H, dh, k_add=ka)
        assert torch.equal(one, full[p * tq:(p + 1) * tq]), p


@pytest.mark.parametrize("tq,tk", [(7, 100), (100, 7)])
def test_cross_attention_reads_column_slices_in_place(tq, tk):
    """q, k and v as column slices of [rows, 384] buffers (the stacked projection), the output a slice of a wider buffer
    between canary columns: the bits of contiguous copies, nothing outside the slice written"""
    from vdr import ops
    H, dh, P = 8, 16, 3
    kv = _bf(_rand((P * tk, 384), 31))
    qb = _bf(_rand((P * tq, 384), 32))
    q, k, v = qb[:, 256:384], kv[:, 0:128], kv[:, 128:256]
    want = ops.cross_attention(q.contiguous(), k.contiguous(), v.contiguous(), P, tq, tk, H, dh)
    whole, body = mg.guarded_rows(P * tq, 384, torch.bfloat16)
    got = ops.cross_attention(q, k, v, P, tq, tk, H, dh, out=body[:, 128:256])
    torch.cuda.synchronize()
    assert torch.equal(got, want) and mg.rows_intact(whole, 8)
    assert mg.canary_left(body[:, :128].contiguous()) == P * tq * 128 and mg.canary_left(body[:, 256:].contiguous()) == P * tq * 128


# ---- the token-side linear (the ReLU path) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,groups", [(35, 128, 256, 1), (21, 256, 2048, 1), (20, 32, 256, 4), (1, 4, 256, 1), (7, 300, 64, 1)])
def test_token_linear_relu_is_max0_of_the_bias_bits_and_both_stay_inside_the_bound(M, N, K, groups):
    from vdr import ops
    x, W = _rand((M, K), 41), _rand((groups, N, K), 42, 1.0 / K ** 0.5)
    b = torch.randn((groups, N), generator=torch.Generator().manual_seed(43))
    Wd = W.to(DEV) if groups > 1 else W[0].to(DEV)
    whole, body = mg.guarded_rows(M, N, torch.bfloat16)
    plain = ops.token_linear(x.to(DEV), Wd, b.to(DEV), out=body)
    relu = ops.token_linear(x.to(DEV), Wd, b.to(DEV), relu=True)
    torch.cuda.synchronize()
    assert mg.rows_intact(whole, 8) and mg.canary_left(body) == 0
    assert torch.equal(relu.view(torch.int16), torch.clamp_min(plain.float(), 0.0).to(torch.bfloat16).view(torch.int16))   # bit for bit
    y, bound = R.token_linear_ref(x, W, b, groups=groups)
    assert R.within_bf16_of(plain, y, bound)
    # bf16(x + x_add) as the input, a residual, fp32 out, strided x rows
    xa, rs = _rand((M, K), 44), _rand((M, N), 45)
    wide = _bf(torch.cat([x, _rand((M, 64), 46)], dim=1))
    got = ops.token_linear(wide[:, :K], Wd, b.to(DEV), x_add=xa.to(DEV), resid=rs.to(DEV), relu=True, out_dtype=torch.float32)
    y, bound = R.token_linear_ref(x, W, b, x_add=xa, resid=rs, relu=True, groups=groups)
    err = (got.double().cpu() - y).abs()
    print(f"token_linear {M}x{N}x{K} groups {groups}: max err / bound {float((err / (bound + 1e-30)).max()):.3f}")
    assert bool((err <= bound + R.U32 * y.abs()).all())


# ---- the upscale tail ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,P", [(1, 1), (3, 2), (10, 3), (64, 1)])
@pytest.mark.parametrize("gelu_in", [False, True])
def test_mask_upscale_stays_inside_its_bound(g, P, gelu_in):
    """g = 1 and 3: 4 and 36 rows, far below one 32-row wave tile; g = 10: 1200 rows, a ragged last tile and tiles that span
    two problems; g = 64: 16384 rows"""
    from vdr import ops
    rows = P * g * g * 4
    x = _rand((rows, 64), 51)
    W = _rand((128, 64), 52, 0.125)
    b = torch.randn(32, generator=torch.Generator().manual_seed(53)) * 0.1
    hy = torch.randn((P, 4, 32), generator=torch.Generator().manual_seed(54))
    whole, body = mg.guarded(P * 4 * 16 * g * g * 4, 4096)
    out = body.view(torch.float32).view(P, 4, 4 * g, 4 * g)
    ops.mask_upscale(x.to(DEV), W.to(DEV), b.to(DEV), hy.to(DEV), P, g, gelu_in=gelu_in, out=out)
    torch.cuda.synchronize()
    assert mg.guards_intact(whole, 4096) and mg.canary_left(out.reshape(-1)) == 0
    want, bound = R.mask_upscale_ref(x, W, b, hy, P, g, gelu_in)
    err = (out.double().cpu() - want).abs()
    print(f"mask_upscale g {g} P {P} gelu_in {gelu_in}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, "
          f"logit rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("g,P", [(3, 2), (10, 3)])
def test_mask_upscale_with_a_zero_convolution_is_hyper_dot_gelu_of_the_bias_exactly(g, P):
    """W = 0: every pre-activation is the bias.  The device polynomial gives gelu(0) = 0 and, beyond its clamp at 5.7 where
    x Phi(-x) is below half an ulp of x, gelu(8) = 8 and gelu(16) = 16 exactly (csrc/vdr_dev.h); with integer hyper the logits
    are integers, exact in any order: the bias add, the activation, the contraction and the scatter bit for bit, asymmetric
    in mask token, channel and problem"""
    from vdr import ops
    rows = P * g * g * 4
    x = torch.randint(-3, 4, (rows, 64), generator=torch.Generator().manual_seed(61)).to(torch.bfloat16)
    b = torch.tensor([0.0, 8.0, 16.0, 8.0] * 8)
    hy = torch.randint(-4, 5, (P, 4, 32), generator=torch.Generator().manual_seed(62)).float()
    out = ops.mask_upscale(x.to(DEV), torch.zeros((128, 64), dtype=torch.bfloat16, device=DEV), b.to(DEV), hy.to(DEV), P, g, gelu_in=True)
    torch.cuda.synchronize()
    want = (hy * b).sum(-1)[:, :, None, None].expand(P, 4, 4 * g, 4 * g)
    assert torch.equal(out.cpu(), want)


def test_mask_upscale_places_every_pixel():
    """one-hot designs: the weight of sub-pixel s2 passes channel 0 of the row through (x 8: beyond the GELU clamp, exact),
    the rows carry their own index, so each logit names the (row, sub-pixel) it came from"""
    from vdr import ops
    g, P = 3, 2
    rows = P * g * g * 4
    x = torch.zeros((rows, 64))
    x[:, 0] = torch.arange(rows, dtype=torch.float32) + 8.0                   # 8 .. 79: exact in bf16, gelu(x) = x on the device
    W = torch.zeros((4, 32, 64))
    for s2 in range(4):
        W[s2, 0, 0] = 1.0
        W[s2, 1, 1] = 1.0
    x[:, 1] = 0.0
    b = torch.zeros(32)
    b[1] = 8.0
    hy = torch.zeros((P, 4, 32))
    hy[:, :, 0] = 1.0
    hy[:, :, 1] = torch.tensor([0.0, 1.0, 2.0, 3.0])                          # + 8 m: the mask token
    out = ops.mask_upscale(_bf(x), _bf(W.reshape(128, 64)), b.to(DEV), hy.to(DEV), P, g, gelu_in=False).cpu()
    for p in range(P):
        for cy in range(g):
            for cx in range(g):
                for s1 in range(4):
                    r = ((p * g + cy) * g + cx) * 4 + s1
                    for s2 in range(4):
                        Y, X = 4 * cy + 2 * (s1 >> 1) + (s2 >> 1), 4 * cx + 2 * (s1 & 1) + (s2 & 1)
                        for m in range(4):
                            assert out[p, m, Y, X] == r + 8.0 + 8.0 * m, (p, cy, cx, s1, s2, m)


# ---- the decode against the goldens ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(golden_dir):
    return {tag: R.golden_case(golden_dir, tag) for tag in ("g8", "g10")}


@contextlib.contextmanager
def _model(c, name="sam_decoder_test"):
    """the golden's miniature SAM under a temporary ARCHS name: seeded encoder weights + the drawn decoder, transformers' eps"""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(c["cfg"].img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS[name] = hc.sam_config(cfg)
    try:
        w = dict(so.make_weights(cfg, seed=c["wseed"], scale=0.05))
        w.update(c["weights"])
        yield vdr.load_model(name, weights=w, decoder_eps=c["eps"])
    finally:
        del vdr.ARCHS[name]


@pytest.fixture(scope="module")
def models(cases):
    with contextlib.ExitStack() as st:
        yield {tag: st.enter_context(_model(c, "sam_decoder_" + tag)) for tag, c in cases.items()}


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_decode_masks_against_the_transformers_golden(cases, models, tag):
    c, m = cases[tag], models[tag]
    assert m.has_mask_decoder
    multi = m.decode_masks(c["emb"].to(DEV), c["boxes"], multimask=True)
    single = m.decode_masks(c["emb"].to(DEV), c["boxes"])
    torch.cuda.synchronize()
    B, nb, g = c["emb"].shape[0], c["boxes"].shape[1], c["cfg"].g
    assert tuple(multi.low_res_logits.shape) == (B, nb, 3, 4 * g, 4 * g) and tuple(single.low_res_logits.shape) == (B, nb, 1, 4 * g, 4 * g)
    assert multi.low_res_logits.dtype == torch.float32 and tuple(multi.iou.shape) == (B, nb, 3) and tuple(single.iou.shape) == (B, nb, 1)
    lg = torch.cat([single.low_res_logits, multi.low_res_logits], dim=2)
    iou = torch.cat([single.iou, multi.iou], dim=2)
    rel, mx, di = R.diffs(lg, iou, c["all4"], c["iou4"])
    g_rel, g_abs, g_iou = (2.0 * v for v in c["bf16_diff"])
    print(f"decode {tag}: relL2 {rel:.3e} (gate {g_rel:.3e})  max|d| {mx:.3e} (gate {g_abs:.3e})  iou head {di:.3e} (gate {g_iou:.3e})")
    assert rel <= g_rel and mx <= g_abs and di <= g_iou
    # the masks: IoU 1 over the pixels whose golden logit is further from 0 than the absolute gate; at most 10 % left out
    clear = c["all4"].abs() > g_abs
    assert float((~clear).double().mean()) <= 0.10
    got, want = (lg.cpu() > 0)[clear], (c["all4"] > 0)[clear]
    assert torch.equal(got, want)
    # the public accessors
    up = single.logits()
    assert tuple(up.shape) == (B, nb, 1, c["cfg"].img, c["cfg"].img)
    ref = torch.nn.functional.interpolate(single.low_res_logits.flatten(0, 1), size=(c["cfg"].img,) * 2, mode="bilinear", align_corners=False)
    assert torch.equal(up.flatten(0, 1), ref) and torch.equal(single.masks(), up > 0) and single.masks(size=(50, 70)).shape[-2:] == (50, 70)


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_segment_image_to_mask_against_the_golden(cases, models, tag):
    """the whole path: the encoder's parity is tests/model_gates.py's, checked on the embedding; the outputs are gated by the
    composition  |device - golden| <= |decoder error on the device's embedding| + |effect of the embedding's error|:  the
    decoder's gate (twice the bf16 mode's difference) plus twice the effect the encoder's bf16-emulating restatement has on
    the float64 decoder restatement -- both measured on the CPU by the generator, stored in the golden file"""
    import model_gates as G
    c, m = cases[tag], models[tag]
    x = c["image"].to(DEV)
    emb = m.image_encoder(x)
    G.check_parity(emb.permute(0, 2, 3, 1), c["emb"].permute(0, 2, 3, 1), f"embedding {tag}", G.gate_l2(2))
    seg = m.segment(x, c["boxes"], multimask=True)
    rel, mx, di = R.diffs(seg.low_res_logits, seg.iou, c["all4"][:, :, 1:], c["iou4"][:, :, 1:])
    g_rel, g_abs, g_iou = (2.0 * (a + b) for a, b in zip(c["bf16_diff"], c["enc_effect"]))
    print(f"segment {tag}: relL2 {rel:.3e} (gate {g_rel:.3e})  max|d| {mx:.3e} (gate {g_abs:.3e})  iou head {di:.3e} (gate {g_iou:.3e})")
    assert rel <= g_rel and mx <= g_abs and di <= g_iou


def test_bitwise_properties_of_the_public_calls(cases, models):
    c, m = cases["g10"], models["g10"]
    x, boxes = c["image"].to(DEV), c["boxes"]
    emb = m.image_encoder(x)
    a = m.segment(x, boxes, multimask=True)
    b = m.decode_masks(emb, boxes, multimask=True)
    assert torch.equal(a.low_res_logits, b.low_res_logits) and torch.equal(a.iou, b.iou)              # segment = encoder + decode
    again = m.decode_masks(emb, boxes, multimask=True)
    assert torch.equal(again.low_res_logits, b.low_res_logits) and torch.equal(again.iou, b.iou)      # two runs
    single = m.decode_masks(emb, boxes)
    lg4, iou4 = m.mask_decoder.decode(emb, boxes)
    assert torch.equal(single.low_res_logits, lg4[:, :, :1]) and torch.equal(b.low_res_logits, lg4[:, :, 1:])   # token 0 / 1..3 of one decode
    assert torch.equal(single.iou, iou4[:, :, :1]) and torch.equal(b.iou, iou4[:, :, 1:])
    for j in range(boxes.shape[1]):                                                                   # nb = 3 is three nb = 1 calls
        one = m.decode_masks(emb, boxes[:, j:j + 1], multimask=True)
        assert torch.equal(one.low_res_logits[:, 0], b.low_res_logits[:, j]) and torch.equal(one.iou[:, 0], b.iou[:, j]), j
    c8, m8 = cases["g8"], models["g8"]                                                                # a batch is its images alone
    e8 = c8["emb"].to(DEV)
    both = m8.decode_masks(e8, c8["boxes"], multimask=True)
    for i in range(2):
        one = m8.decode_masks(e8[i:i + 1], c8["boxes"][i:i + 1], multimask=True)
        assert torch.equal(one.low_res_logits[0], both.low_res_logits[i]) and torch.equal(one.iou[0], both.iou[i]), i


def test_segment_volume_returns_the_mask_generate_features_takes(cases, models):
    import vdr
    c, m = cases["g8"], models["g8"]
    H, W, S = 96, 80, 5
    vol = torch.rand((H, W, S), generator=torch.Generator().manual_seed(71)).numpy().astype(np.float32)
    box = np.array([20.0, 25.0, 60.0, 70.0])
    mask = vdr.pipeline.segment_volume(m, vol, box, max_batch=2)
    assert mask.shape == (H, W, S) and mask.dtype == np.bool_
    per = vdr.pipeline.segment_volume(m, vol, np.tile(box, (S, 1)), max_batch=2)
    assert np.array_equal(mask, per)                                          # one box for all slices = the same box per slice
    # the slice call is the volume call run slice by slice (chunks of one: the same encoder batch; the decode itself does not
    # depend on the batch -- test_bitwise_properties_of_the_public_calls)
    alone = vdr.pipeline.segment_volume(m, vol, box, max_batch=1)
    one = vdr.segment_slice(m, vol[:, :, 3], box)
    assert one.shape == (H, W) and one.dtype == np.bool_ and np.array_equal(one, alone[:, :, 3])
    if not mask.any():                                                         # (random weights: any mask will do for the plumbing)
        mask[30:50, 30:50, :] = True
    feats, masks = vdr.pipeline.generate_features(m, vol, mask)
    assert len(feats) == S and len(masks) == S and feats[0].shape[-1] == 256


# ---- the decoder object: what load_model keeps, the handle's weight list, the memory contract --------------------------------
def test_an_encoder_only_checkpoint_loads_without_a_decoder_and_segment_refuses(cases):
    import vdr
    from oracle import sam_oracle as so
    c = cases["g8"]
    cfg = so.SamCfg(128, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS["sam_encoder_only"] = hc.sam_config(cfg)
    try:
        m = vdr.load_model("sam_encoder_only", weights=so.make_weights(cfg, seed=c["wseed"], scale=0.05))
    finally:
        del vdr.ARCHS["sam_encoder_only"]
    assert m.has_mask_decoder is False and m.mask_decoder is None
    x = c["image"].to(DEV)
    emb = m.image_encoder(x)                                                   # everything that worked still works
    assert tuple(emb.shape) == (2, 256, 8, 8) and bool(torch.isfinite(emb).all())
    with pytest.raises(ValueError, match="encoder-only"):
        m.segment(x, c["boxes"])
    with pytest.raises(ValueError, match="encoder-only"):
        m.decode_masks(emb, c["boxes"])
    with pytest.raises(ValueError, match="encoder-only"):
        vdr.segment_slice(m, np.zeros((20, 30), np.float32), [1, 2, 10, 12])


def test_the_handle_enumerates_segment_anythings_names(models):
    import ctypes as C
    d = models["g8"].mask_decoder
    names = [d.lib.vdr_mask_decoder_weight_name(d.h, i).decode() for i in range(d.lib.vdr_mask_decoder_num_weights(d.h))]
    shapes = R.decoder_shapes(128)
    assert len(names) == len(set(names)) and set(names) == set(shapes) - {"prompt_encoder.point_embeddings.0.weight", "prompt_encoder.point_embeddings.1.weight"}
    assert d.lib.vdr_mask_decoder_weight_name(d.h, len(names)) is None and d.lib.vdr_mask_decoder_weight_name(d.h, -1) is None
    buf = torch.zeros(8)
    assert d.lib.vdr_mask_decoder_set_weight(d.h, b"mask_decoder.iou_token.weight", buf.data_ptr(), (C.c_int64 * 1)(8), 1) == -1   # finalized
    n1, n3 = d.workspace_bytes(1), d.workspace_bytes(3)
    assert 0 < n1 < n3 and n1 % 256 == 0


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_decode_memory_contract(cases, models, tag):
    """a workspace one byte short is refused (VDR_ERR_WORKSPACE) with nothing written -- workspace, logits and IoU keep their
    canaries; in a workspace of exactly the stated size the decode gives the bits of any other decode and touches no byte
    past it, nor around its outputs"""
    import vdr
    c, m = cases[tag], models[tag]
    d = m.mask_decoder
    emb, boxes = c["emb"].to(DEV), c["boxes"].to(DEV).float().contiguous()
    B, nb, g = emb.shape[0], boxes.shape[1], d.g
    P = B * nb
    need = d.workspace_bytes(P)
    whole, body = mg.guarded(need, 4096)
    lw, lb = mg.guarded(P * 4 * 16 * g * g * 4, 4096)
    iw, ib = mg.guarded(P * 4 * 4, 4096)
    embc = emb.contiguous()

    def call(nbytes):
        return d.lib.vdr_mask_decode(d.h, embc.data_ptr(), 0, boxes.data_ptr(), B, nb, body.data_ptr(), nbytes, lb.data_ptr(), ib.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert call(need - 1) == -5 and b"workspace too small" in d.lib.vdr_last_error(None)
    torch.cuda.synchronize()
    for t in (whole, lw, iw):
        assert bool((t == mg.CANARY).all())                                    # nothing written anywhere
    assert call(need) == 0
    torch.cuda.synchronize()
    assert mg.guards_intact(whole, 4096) and mg.guards_intact(lw, 4096) and mg.guards_intact(iw, 4096)
    lg, iou = d.decode(emb, c["boxes"])
    assert torch.equal(lb.view(torch.float32).view(lg.shape), lg) and torch.equal(ib.view(torch.float32).view(iou.shape), iou)
    assert mg.canary_left(lb.view(torch.float32)) == 0 and mg.canary_left(ib.view(torch.float32)) == 0
    # the encoder's own channel-last layout is read in place: the same bits as the channel-first copy
    lg2, iou2 = d.decode(emb.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), c["boxes"])
    assert torch.equal(lg2, lg) and torch.equal(iou2, iou)


def test_a_whole_checkpoint_in_transformers_spelling_loads_to_the_same_bits(cases, models):
    """encoder and decoder both spelled as transformers.SamModel's state dict spells them"""
    import vdr
    from oracle import sam_oracle as so
    c = cases["g8"]
    cfg = so.SamCfg(128, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    sd = dict(R.encoder_to_hf(so.make_weights(cfg, seed=c["wseed"], scale=0.05)))
    sd.update(R.to_hf(c["weights"]))
    assert not any(k.startswith(("blocks.", "image_encoder.", "mask_decoder.output_upscaling")) for k in sd)
    vdr.ARCHS["sam_hf_spelled"] = hc.sam_config(cfg)
    try:
        m = vdr.load_model("sam_hf_spelled", weights=sd, decoder_eps=c["eps"])
    finally:
        del vdr.ARCHS["sam_hf_spelled"]
    assert m.has_mask_decoder
    x = c["image"].to(DEV)
    a, b = m.segment(x, c["boxes"], multimask=True), models["g8"].segment(x, c["boxes"], multimask=True)
    assert torch.equal(a.low_res_logits, b.low_res_logits) and torch.equal(a.iou, b.iou)
