"""GPU parity of the full forward path through the C ABI (vdr_forward / vdr_forward_tokens) against
the CPU fp32 oracle and the committed golden vectors.

Stated tolerances (SURVEY.md §8d "Parity gate"), for a model of L layers:
  * bf16 HIP path vs the fp32 oracle on identical seeded inputs: per-row cosine >= 0.999 and
    relative L2 <= gate(L) = 4e-3 + 3e-3*sqrt(L)  (9.2e-3 at L=3, 1.44e-2 at L=12).  bf16 keeps 8
    significant bits (2^-9 relative per rounding); every block rounds the residual stream, the
    normalised activations, q/k/v, P, the attention output and the MLP hidden once, and the
    roundings add in quadrature over L blocks — measured 5.5e-3 (L=2) ... 9.6e-3 (L=12);
  * bf16 HIP path vs the oracle run with bf16 rounding EMULATED at the same store points: same
    gate.  It cannot be much tighter: the two paths sum in different orders, so values that sit near
    a bf16 rounding boundary round differently and the two error patterns decorrelate; the check
    still shows that no error beyond the precision choice is present (per-kernel tests in
    test_ops_gpu.py pin each kernel to one bf16 rounding of an fp32 reference);
  * golden vectors produced by the reference's own TransformerNoduleClassifier: same gates.
"""
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
from model_gates import check_parity, check_parity_fp8, gate_l2, gate_l2_fp8, inject_outlier_channels, min_cos, rel_l2
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


SMALL = {
    "tiny_p8": hc.TINY,
    "p16_d128": vo.VitCfg(64, 16, 3, 128, 2, 3, 512),
    "p14_d192": vo.VitCfg(56, 14, 3, 192, 3, 2, 768),
    "dinov2_swiglu_ls": vo.VitCfg(56, 14, 3, 128, 2, 2, 320 + 64, act="swiglu", layerscale=True),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_vit_all_outputs(name):
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 5, seed=4)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    xd = x.cuda()
    g = gate_l2(cfg.layers)
    check_parity(e.forward(xd, vdr.OUT_CLS), ref["cls"], f"{name} cls", g, emu["cls"])
    check_parity(e.forward(xd, vdr.OUT_DENSE), ref["dense"], f"{name} dense", g, emu["dense"])
    check_parity(e.forward(xd, vdr.OUT_TOKENS), ref["tokens"], f"{name} tokens", g, emu["tokens"])
    check_parity(e.forward(xd, vdr.OUT_PATCH_EMBED), ref["patch_embed"], f"{name} patch_embed", 4e-3, emu["patch_embed"])
    # bf16 input images and bf16 outputs take the same path
    d16 = e.forward(xd.to(torch.bfloat16), vdr.OUT_DENSE, torch.bfloat16)
    assert d16.dtype == torch.bfloat16 and rel_l2(d16.float().cpu(), ref["dense"]) < 3e-2


def test_first_forward_after_finalize_is_graph_capturable():
    """include/vdr.h: the hot-path calls never synchronise, allocate or copy from the host.  The FIRST vdr_forward after
    load (vdr_finalize did the load-time work) is captured into a HIP graph -- a hipMalloc / hipMemcpy /
    hipDeviceSynchronize inside it would fail the capture -- and the replay reproduces an eager forward bit for bit."""
    import vdr
    cfg = SMALL["p16_d128"]
    vcfg = vdr.VdrConfig(img=cfg.img, patch=cfg.patch, in_chans=cfg.in_chans, dim=cfg.dim, heads=cfg.heads, layers=cfg.layers,
                         mlp_hidden=cfg.mlp_hidden)
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 5, seed=2).cuda()
    e = vdr.Engine(vcfg)
    with pytest.raises(vdr.VdrError):  # nothing loaded, not finalised: an error, not a lazy resolve
        e.forward(x, vdr.OUT_CLS)
    e.load_weights(w)  # ends with vdr_finalize
    out = torch.empty((5, cfg.dim), dtype=torch.float32, device="cuda")
    e._workspace(5)  # the caller-owned workspace exists before the capture (torch allocation, not the library's)
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
    eager = vdr.Engine(vcfg)
    eager.load_weights(w)
    assert torch.equal(out, eager.forward(x, vdr.OUT_CLS))


def test_micro_batching_does_not_change_results():
    import vdr
    cfg = SMALL["p16_d128"]
    w = vo.make_weights(cfg, seed=5, scale=0.05)
    x = vo.make_images(cfg, 7, seed=6).cuda()
    a = hc.engine(cfg, w).forward(x, vdr.OUT_CLS)
    b = hc.engine(cfg, w, micro_batch=3).forward(x, vdr.OUT_CLS)
    assert torch.equal(a, b)
    one = hc.engine(cfg, w).forward(x[2:3], vdr.OUT_CLS)
    assert torch.equal(a[2:3], one), "a row must not depend on what else is in the batch"


def test_vit_tiny16_224_config1():
    """BASELINE config 1 geometry (ViT-Ti/16 224^2, batch 8 -> [8,192] CLS) on the GPU vs the oracle."""
    import vdr
    cfg = vo.CONFIGS["vit_tiny16_224"]
    w = vo.make_weights(cfg, seed=1)
    x = vo.make_images(cfg, 8, seed=0)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    got = e.forward(x.cuda(), vdr.OUT_CLS)
    assert got.shape == (8, 192) and got.dtype == torch.float32
    check_parity(got, ref["cls"], "vit_tiny cls", gate_l2(12), emu["cls"])
    check_parity(e.forward(x.cuda(), vdr.OUT_DENSE), ref["dense"], "vit_tiny dense", gate_l2(12), emu["dense"])


def test_vit_base16_224_headline_config():
    """BASELINE config 2 geometry (ViT-B/16 224^2); batch 4 keeps the CPU oracle to seconds."""
    import vdr
    cfg = vo.CONFIGS["vit_base16_224"]
    w = vo.make_weights(cfg, seed=1)
    x = vo.make_images(cfg, 4, seed=0)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    got = e.forward(x.cuda().to(torch.bfloat16), vdr.OUT_CLS)
    assert got.shape == (4, 768)
    check_parity(got, ref["cls"], "vit_base cls", gate_l2(12), emu["cls"])


def test_vit_large14_336_geometry_dense_tokens():
    """BASELINE config 4 geometry (ViT-L/14 336^2: 577 tokens -> online-softmax attention, D=1024,
    H=16, F=4096), depth cut to 2 blocks so the CPU oracle stays in seconds; dense per-patch tokens."""
    import vdr
    full = vo.CONFIGS["vit_large14_336"]
    cfg = vo.VitCfg(full.img, full.patch, 3, full.dim, full.heads, 2, full.mlp_hidden)
    w = vo.make_weights(cfg, seed=4)
    x = vo.make_images(cfg, 2, seed=5)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    dense = e.forward(x.cuda().to(torch.bfloat16), vdr.OUT_DENSE, torch.bfloat16)
    assert dense.shape == (2, 576, 1024) and dense.dtype == torch.bfloat16
    check_parity(dense, ref["dense"], "vit_large14 dense (bf16 out)", gate_l2(2) + 2e-3, emu["dense"])
    check_parity(e.forward(x.cuda(), vdr.OUT_CLS), ref["cls"], "vit_large14 cls", gate_l2(2), emu["cls"])


def test_dinov2_giant14_geometry_swiglu_layerscale():
    """BASELINE config 5 geometry in bf16 (DINOv2 ViT-g/14: D=1536, H=24, SwiGLU hidden 4096, LayerScale,
    257 tokens -> 9 key tiles), depth cut to 2 blocks."""
    import vdr
    full = vo.CONFIGS["dinov2_giant14_224"]
    cfg = vo.VitCfg(full.img, full.patch, 3, full.dim, full.heads, 2, full.mlp_hidden, act="swiglu", layerscale=True)
    w = vo.make_weights(cfg, seed=6)
    x = vo.make_images(cfg, 3, seed=7)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    check_parity(e.forward(x.cuda(), vdr.OUT_CLS), ref["cls"], "dinov2_giant14 cls", gate_l2(2), emu["cls"])
    check_parity(e.forward(x.cuda(), vdr.OUT_DENSE), ref["dense"], "dinov2_giant14 dense", gate_l2(2), emu["dense"])


@pytest.mark.parametrize("name", ["p16_d128", "p14_d192", "dinov2_swiglu_ls"])
def test_fp8_small_vit_all_outputs(name):
    """BASELINE config 5 path (MX-fp8 qkv / fc1 / fc2 on the block-scaled MFMA) on the small geometries."""
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 5, seed=4)
    ref = vo.forward_images(cfg, w, x)
    xd = x.cuda()
    for level, mode in ((1, "mx"),):
        emx = vo.forward_images(cfg, w, x, emulate_bf16=mode)
        e = hc.engine(cfg, w, fp8=level)
        check_parity_fp8(e.forward(xd, vdr.OUT_CLS), ref["cls"], emx["cls"], cfg.layers, f"{name} fp8={level} cls")
        check_parity_fp8(e.forward(xd, vdr.OUT_DENSE), ref["dense"], emx["dense"], cfg.layers, f"{name} fp8={level} dense")
    # the fp8 path is still batch-independent and deterministic
    a = e.forward(xd, vdr.OUT_CLS)
    b = e.forward(xd[[3, 1, 4, 0, 2]], vdr.OUT_CLS)
    assert torch.equal(a[[3, 1, 4, 0, 2]], b)


def test_fp8_dinov2_giant14_config5_geometry():
    """BASELINE config 5: DINOv2 ViT-g/14 (D=1536, H=24, SwiGLU 4096, LayerScale, 257 tokens) with fp8 weights,
    depth cut to 2 blocks for the oracle's sake; plus ViT-B/16 dims (GELU) at 3 blocks."""
    import vdr
    full = vo.CONFIGS["dinov2_giant14_224"]
    for cfg, tag in [(vo.VitCfg(full.img, full.patch, 3, full.dim, full.heads, 2, full.mlp_hidden, act="swiglu", layerscale=True), "vitg"),
                     (vo.VitCfg(224, 16, 3, 768, 12, 3, 3072), "vitb")]:
        w = vo.make_weights(cfg, seed=6)
        x = vo.make_images(cfg, 3, seed=7)
        ref = vo.forward_images(cfg, w, x)
        for level, mode in ((1, "mx"),):
            emx = vo.forward_images(cfg, w, x, emulate_bf16=mode)
            e = hc.engine(cfg, w, fp8=level)
            check_parity_fp8(e.forward(x.cuda(), vdr.OUT_CLS), ref["cls"], emx["cls"], cfg.layers, f"{tag} fp8={level} cls")
            check_parity_fp8(e.forward(x.cuda(), vdr.OUT_DENSE), ref["dense"], emx["dense"], cfg.layers,
                             f"{tag} fp8={level} dense")


def test_fp8_is_refused_where_it_is_not_implemented():
    import vdr
    with pytest.raises(RuntimeError):
        vdr.Engine(vdr.VdrConfig(img=0, patch=0, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False, has_pos=False,
                                 input_ln=True, fp8=True))


def test_layernorm_folding_matches_the_explicit_layernorm_path():
    """Pre-LN image models fold LayerNorm into the qkv / fc1 GEMMs (row statistics from the producer's
    epilogue, gamma folded into the weights).  vdr_config.no_ln_fold = 1 keeps the explicit LayerNorm kernel: both
    paths must agree to bf16 noise, also when the token rows carry a mean several sigma away from 0
    (variance is formed as E[x^2] - mean^2 from fp32 partial sums)."""
    import vdr
    cfg = SMALL["p14_d192"]
    w = vo.make_weights(cfg, seed=12, scale=0.05)
    w["pos_embed"] = w["pos_embed"] + 1.5          # rows with |mean| >> their spread
    x = vo.make_images(cfg, 6, seed=13)
    ref = vo.forward_images(cfg, w, x)
    fused = hc.engine(cfg, w).forward(x.cuda(), vdr.OUT_TOKENS)
    plain = hc.engine(cfg, w, ln_fold=False).forward(x.cuda(), vdr.OUT_TOKENS)
    assert not torch.equal(fused, plain)  # two different code paths really ran
    # rows with mean 1.5 keep fewer bf16 bits for their spread: both paths sit ~1.5x above the usual gate
    g = 1.5 * gate_l2(cfg.layers)
    r_f, r_p = rel_l2(fused.cpu(), ref["tokens"]), rel_l2(plain.cpu(), ref["tokens"])
    print(f"LN fold: fused {r_f:.3e}  explicit {r_p:.3e}  fused-vs-explicit {rel_l2(fused.cpu(), plain.cpu()):.3e}")
    assert r_f <= g and r_p <= g
    assert r_f <= 1.25 * r_p, "folding LayerNorm must not cost accuracy"
    assert rel_l2(fused.cpu(), plain.cpu()) <= g
    assert min_cos(fused.cpu(), ref["tokens"]) >= 0.999


def test_outlier_channels_vit_g_geometry():
    """DINOv2 ViT-g/14 geometry (1536 / 24 heads / SwiGLU 4096 / LayerScale) at 4 blocks with outlier channels injected:
    bf16 with the LayerNorm fold on and off and MX-fp8 weights, against the fp32 oracle under the usual gates."""
    import vdr
    big = vo.CONFIGS["dinov2_giant14_224"]
    cfg = vo.VitCfg(big.img, big.patch, 3, big.dim, big.heads, 4, big.mlp_hidden, act=big.act, layerscale=True)
    w, ch = inject_outlier_channels(vo.make_weights(cfg, seed=31), cfg.layers, cfg.dim, 32, "mlp.w12")
    x = vo.make_images(cfg, 2, seed=33)
    ref = vo.forward_images(cfg, w, x)
    # the injection does what it says: the residual stream carries the two channels at 10^2..10^3 in every token
    assert ref["tokens"].shape[-1] == cfg.dim
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    g = gate_l2(cfg.layers)
    fused = hc.engine(cfg, w).forward(x.cuda(), vdr.OUT_TOKENS)
    plain = hc.engine(cfg, w, ln_fold=False).forward(x.cuda(), vdr.OUT_TOKENS)
    assert not torch.equal(fused, plain)
    check_parity(fused, ref["tokens"], "outliers ViT-g L4 bf16, LayerNorm folded", g, emu["tokens"])
    check_parity(plain, ref["tokens"], "outliers ViT-g L4 bf16, explicit LayerNorm", g, emu["tokens"])
    assert rel_l2(fused.cpu(), ref["tokens"]) <= 1.25 * rel_l2(plain.cpu(), ref["tokens"]) + 1e-3, "the fold must not cost accuracy on outlier rows"
    # MX-fp8.  Analysed on the CPU with the MX-emulating oracle (the same quantisation points in plain torch fp32:
    # tools/fp8_outlier_analysis.py, profiles/r04_fp8_outlier_analysis.txt), which shows the same numbers as the kernels.
    # Gain outliers alone cost nothing (min cos 0.99724 with, 0.99731 without: e4m3 is a floating-point format).  Residual
    # channels at +300 / -120 in every PATCH token take the CLS rows -- the only rows without them -- from 0.9973 to 0.9895.
    # Not through those channels' own products (their activations AND weight columns kept exact: 0.9902; a hi + lo split
    # of both: 0.9902), and not through the patch rows at all (patch rows quantised, CLS rows not: 0.99993): LayerNorm
    # scales the other channels of a patch row down 8x, the attention update of the CLS row shrinks from |23| to |2.9|
    # per block, and the CLS row ends up made of its OWN MLP outputs (|18| per block) -- an MX-fp8 MLP chain is ~13 %
    # relative error per block (LN2 out 2.8e-3, w12 2.6e-3, u 1.5e-3, w3 1.4e-3 of 1 - cos) with nothing to average it
    # out.  It grows with depth (emulation, 40 blocks: 0.919).  The remedy that works is precision for the CLS rows' own
    # MLP: vdr_config.fp8_cls_bf16 (below; emulation 0.9986 at 4 blocks, 0.9886 at 40).  Without it this stress case is
    # gated at 0.985 and on agreement with the emulating oracle (a stated deviation: include/vdr.h).
    emx = vo.forward_images(cfg, w, x, emulate_bf16="mx")
    f8 = hc.engine(cfg, w, fp8=1).forward(x.cuda(), vdr.OUT_TOKENS).float().cpu()
    assert torch.isfinite(f8).all()
    r32, rmx = rel_l2(f8, ref["tokens"]), rel_l2(f8, emx["tokens"])
    cos = torch.nn.functional.cosine_similarity(f8.double().reshape(-1, cfg.dim), ref["tokens"].double().reshape(-1, cfg.dim), dim=-1)
    cos_emx = min_cos(emx["tokens"], ref["tokens"])
    n_tok = ref["tokens"].shape[1]
    patch_rows = torch.ones(cos.numel(), dtype=torch.bool)
    patch_rows[::n_tok] = False  # row 0 of every image is its CLS token
    print(f"outliers ViT-g L4 MX-fp8: relL2 vs fp32 {r32:.3e}  vs MX-emulating oracle {rmx:.3e}  min cos CLS rows {cos[~patch_rows].min():.6f} "
          f"(MX-emulating oracle {cos_emx:.6f})  patch rows {cos[patch_rows].min():.6f}")
    gate = gate_l2_fp8(cfg.layers)
    assert r32 <= gate and rmx <= gate
    assert cos[patch_rows].min() >= 0.99
    assert cos[~patch_rows].min() >= 0.985 and abs(cos[~patch_rows].min().item() - cos_emx) <= 5e-3
    # vdr_config.fp8_cls_bf16: the CLS rows' MLP on the bf16 weights -> back above the stated gate of the fp8 path
    vo.MX_CLS_MLP_BF16 = True
    try:
        emc = vo.forward_images(cfg, w, x, emulate_bf16="mx")
    finally:
        vo.MX_CLS_MLP_BF16 = False
    f8c = hc.engine(cfg, w, fp8=1, fp8_cls_bf16=True).forward(x.cuda(), vdr.OUT_TOKENS).float().cpu()
    assert torch.isfinite(f8c).all()
    cosc = torch.nn.functional.cosine_similarity(f8c.double().reshape(-1, cfg.dim), ref["tokens"].double().reshape(-1, cfg.dim), dim=-1)
    cosc_emu = torch.nn.functional.cosine_similarity(emc["tokens"].double().reshape(-1, cfg.dim), ref["tokens"].double().reshape(-1, cfg.dim), dim=-1)
    print(f"outliers ViT-g L4 MX-fp8 + fp8_cls_bf16: min cos CLS rows {cosc[~patch_rows].min():.6f} (emulating oracle "
          f"{cosc_emu[~patch_rows].min():.6f})  patch rows {cosc[patch_rows].min():.6f}  relL2 vs emulation {rel_l2(f8c, emc['tokens']):.3e}")
    assert cosc[~patch_rows].min() >= 0.99 and cosc[patch_rows].min() >= 0.99
    assert abs(cosc[~patch_rows].min().item() - cosc_emu[~patch_rows].min().item()) <= 2e-3
    assert rel_l2(f8c, emc["tokens"]) <= gate


def test_outlier_channels_medsam_geometry():
    """The same injection on the SAM ViT-B@1024 encoder at 3 blocks (window, window, global), one slice."""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(layers=3, global_idx=(2,))
    w, ch = inject_outlier_channels(so.make_weights(cfg, seed=41), cfg.layers, cfg.dim, 42, "mlp.fc1")
    x = so.make_images(cfg, 1, seed=43)
    ref = so.sam_forward(cfg, w, x)
    emu = so.sam_forward(cfg, w, x, emulate_bf16=True)
    gr = cfg.grid
    tok = hc.sam_engine(cfg, w).forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity(tok, ref["tokens"].reshape(1, gr * gr, cfg.dim), "outliers MedSAM L3 bf16 tokens", gate_l2(cfg.layers),
                 emu["tokens"].reshape(1, gr * gr, cfg.dim))
    emx = so.sam_forward(cfg, w, x, emulate_bf16="mx")
    t8 = hc.sam_engine(cfg, w, fp8=1).forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity_fp8(t8, ref["tokens"].reshape(1, gr * gr, cfg.dim), emx["tokens"].reshape(1, gr * gr, cfg.dim), cfg.layers,
                     "outliers MedSAM L3 MX-fp8 tokens")


@pytest.mark.parametrize("name", ["p16_d128", "p14_d192", "dinov2_swiglu_ls"])
@pytest.mark.parametrize("cls_bf16", [False, True])
def test_cls_rows_only_last_block_bitwise_fp8(name, cls_bf16):
    """The same short cut on the MX-fp8 path (BASELINE config 5): norm2 of the CLS rows is quantised on its own, fc1 / fc2
    run on the block-scaled MFMA at M = batch -- the features must still be the bits of the full block.  With
    vdr_config.fp8_cls_bf16 the CLS rows' MLP of EVERY block runs on the bf16 weights (side stream, rows put back after
    the MX-fp8 fc2 of all rows): the full block and the CLS tail must still agree bit for bit, the patch rows must be the
    bits of the plain fp8 model's first block ... and the CLS rows must differ from it (the switch does something)."""
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=23, scale=0.05)
    x = vo.make_images(cfg, 7, seed=24).cuda()
    full = hc.engine(cfg, w, fp8=1, full_last_block=True, fp8_cls_bf16=cls_bf16)
    ref_cls = full.forward(x, vdr.OUT_CLS)
    assert torch.equal(ref_cls, full.forward(x, vdr.OUT_TOKENS)[:, 0])
    for mb in (0, 3):
        got = hc.engine(cfg, w, fp8=1, micro_batch=mb, fp8_cls_bf16=cls_bf16).forward(x, vdr.OUT_CLS)
        assert torch.equal(got, ref_cls), f"micro_batch {mb}"
    assert torch.equal(hc.engine(cfg, w, fp8=1, fp8_cls_bf16=cls_bf16).forward(x, vdr.OUT_DENSE), full.forward(x, vdr.OUT_DENSE))
    if cls_bf16:
        plain = hc.engine(cfg, w, fp8=1, full_last_block=True).forward(x, vdr.OUT_CLS)
        assert not torch.equal(plain, ref_cls), "fp8_cls_bf16 changed nothing"
        # three forwards in a row through the side stream: same bits every time (the fork / join events are reused)
        for _ in range(3):
            assert torch.equal(full.forward(x, vdr.OUT_CLS), ref_cls)


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("ln_fold", [True, False])
def test_cls_rows_only_last_block_bitwise(name, ln_fold):
    """VDR_OUT_CLS runs the out-projection / norm2 / MLP of the LAST block on the CLS rows only (after the last attention
    every operation is row-wise; models_archs.py:24-29 keeps x[:, 0]).  The features must be the bits of the full block
    (vdr_config.full_last_block = 1) -- with and without the LayerNorm fold, LayerScale, SwiGLU, micro-batches -- and
    the full block's own CLS output must equal row 0 of its token output (so the comparison is not vacuous)."""
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=21, scale=0.05)
    x = vo.make_images(cfg, 7, seed=22).cuda()
    full = hc.engine(cfg, w, ln_fold=ln_fold, full_last_block=True)
    ref_cls = full.forward(x, vdr.OUT_CLS)
    assert torch.equal(ref_cls, full.forward(x, vdr.OUT_TOKENS)[:, 0])
    for mb in (0, 3):
        got = hc.engine(cfg, w, ln_fold=ln_fold, micro_batch=mb).forward(x, vdr.OUT_CLS)
        assert torch.equal(got, ref_cls), f"micro_batch {mb}"
    # the other outputs never take the short cut
    pruned = hc.engine(cfg, w, ln_fold=ln_fold)
    assert torch.equal(pruned.forward(x, vdr.OUT_TOKENS), full.forward(x, vdr.OUT_TOKENS))
    assert torch.equal(pruned.forward(x, vdr.OUT_DENSE), full.forward(x, vdr.OUT_DENSE))


def test_streams_and_micro_batches_do_not_change_results():
    import vdr
    cfg = SMALL["p14_d192"]
    w = vo.make_weights(cfg, seed=8, scale=0.05)
    x = vo.make_images(cfg, 9, seed=9).cuda()
    a = hc.engine(cfg, w).forward(x, vdr.OUT_DENSE)
    vc = vdr.VdrConfig(img=cfg.img, patch=cfg.patch, dim=cfg.dim, heads=cfg.heads, layers=cfg.layers,
                       mlp_hidden=cfg.mlp_hidden, streams=2, micro_batch=2)
    e2 = vdr.Engine(vc)
    e2.load_weights(w)
    for _ in range(3):
        assert torch.equal(e2.forward(x, vdr.OUT_DENSE), a)


@pytest.mark.parametrize("tag", ["tiny", "refconf", "cfg1"])
def test_golden_reference_class_tokens(golden_dir, tag):
    """models_archs.TransformerNoduleClassifier golden vectors (made by the reference itself)."""
    import vdr
    g = np.load(os.path.join(golden_dir, f"postln_{tag}.npz"), allow_pickle=False)
    dim, heads, layers, ffn = int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"])
    cfg = vo.postln_cfg(dim, heads, layers, ffn)
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = vo.make_tokens(int(g["batch"]), int(g["seq"]), dim, seed=int(g["xseed"]))
    emu = vo.forward_tokens(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    cls = e.forward_tokens(x.cuda(), vdr.OUT_CLS)
    check_parity(cls, torch.from_numpy(g["cls"]), f"golden postln_{tag} cls", gate_l2(layers), emu["cls"])
    # the drop-in class: (logits, cls) tuple, state_dict in the reference's own key names
    sd = {"cls_token": w["cls_token"], "norm.weight": w["input_norm.weight"], "norm.bias": w["input_norm.bias"]}
    for i in range(layers):
        s, d = f"blocks.{i}.", f"transformer_encoder.layers.{i}."
        sd[d + "self_attn.in_proj_weight"] = w[s + "attn.qkv.weight"]
        sd[d + "self_attn.in_proj_bias"] = w[s + "attn.qkv.bias"]
        sd[d + "self_attn.out_proj.weight"] = w[s + "attn.proj.weight"]
        sd[d + "self_attn.out_proj.bias"] = w[s + "attn.proj.bias"]
        sd[d + "linear1.weight"], sd[d + "linear1.bias"] = w[s + "mlp.fc1.weight"], w[s + "mlp.fc1.bias"]
        sd[d + "linear2.weight"], sd[d + "linear2.bias"] = w[s + "mlp.fc2.weight"], w[s + "mlp.fc2.bias"]
        for n in ("norm1", "norm2"):
            sd[d + n + ".weight"], sd[d + n + ".bias"] = w[s + n + ".weight"], w[s + n + ".bias"]
    for k in ("dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias"):
        sd["classifier." + k] = torch.from_numpy(g["head.classifier." + k])
    # the reference's own flow (train_models.py:455-486 build_model, models_archs.py:32-35 load): construct with the
    # reference signature, then load_state_dict(torch.load(path)); calling the model before that is an error
    m = vdr.TransformerNoduleClassifier(input_dim=dim, dim_feedforward=ffn, num_heads=heads, num_classes=2, num_layers=layers)
    with pytest.raises(RuntimeError):
        m(x.cuda())
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    m.load_state_dict(torch.load(buf, map_location="cuda", weights_only=True))
    m = m.to("cuda").eval()
    assert sorted(m.state_dict()) == sorted(sd)
    logits, cls2 = m(x.cuda())
    # the constructor shortcut gives the same model
    m2 = vdr.TransformerNoduleClassifier(dim, ffn, heads, 2, layers, state_dict=sd)
    assert torch.equal(m2(x.cuda())[1], cls2)
    assert logits.shape == (int(g["batch"]), 2) and cls2.shape == (int(g["batch"]), dim)
    assert torch.equal(cls2, cls)
    err = (logits.cpu() - torch.from_numpy(g["logits"])).abs().max().item()
    assert err < 3e-2, f"logits max abs err {err}"


@pytest.mark.parametrize("dims,lens", [((64, 1, 2, 128), [5, 1, 17, 9]),
                                       ((256, 4, 2, 1024), [37, 200, 1, 129, 64, 200]),     # the reference's configured dims
                                       ((192, 3, 2, 768), [300, 20, 513, 64])])              # > 288 tokens: online softmax
def test_variable_length_sequences_match_one_at_a_time(dims, lens):
    """the reference runs its masked-voxel sequences with batch_size 1 because they differ in
    length; padded to the longest and run in ONE call (per-sequence key masking) every CLS row must equal the
    oracle's result for that sequence alone, and the GPU's own one-at-a-time result within kernel-variant noise."""
    import vdr
    dim, heads, layers, ffn = dims
    cfg = vo.postln_cfg(dim, heads, layers, ffn)
    w = vo.make_weights(cfg, seed=13, scale=0.05)
    e = hc.engine(cfg, w)
    S = max(lens)
    seqs = [vo.make_tokens(1, n, dim, seed=100 + i)[0] for i, n in enumerate(lens)]
    pad = torch.full((len(lens), S, dim), 3.0)  # non-zero padding: it must not leak into any valid row
    for i, t in enumerate(seqs):
        pad[i, : t.shape[0]] = t
    got = e.forward_tokens(pad.cuda(), vdr.OUT_CLS, lengths=lens).float().cpu()
    for i, t in enumerate(seqs):
        ref = vo.forward_tokens(cfg, w, t[None])["cls"][0]
        one = e.forward_tokens(t[None].cuda(), vdr.OUT_CLS).float().cpu()[0]
        r_ref = rel_l2(got[i][None], ref[None])
        r_one = rel_l2(got[i][None], one[None])
        assert r_ref <= gate_l2(layers) and r_one <= 4e-3, (i, lens[i], r_ref, r_one)
    # padding content is irrelevant, bitwise
    pad2 = pad.clone()
    for i, t in enumerate(seqs):
        pad2[i, t.shape[0]:] = -7.5
    assert torch.equal(got, e.forward_tokens(pad2.cuda(), vdr.OUT_CLS, lengths=lens).float().cpu())
    # lengths == S everywhere is the fixed-length path
    full = e.forward_tokens(pad.cuda(), vdr.OUT_CLS, lengths=[S] * len(lens)).float().cpu()
    assert rel_l2(full, e.forward_tokens(pad.cuda(), vdr.OUT_CLS).float().cpu()) <= 4e-3
    with pytest.raises(ValueError):
        e.forward_tokens(pad.cuda(), vdr.OUT_CLS, lengths=[0] + lens[1:])


@pytest.mark.parametrize("name", ["vit_hf_tiny", "vit_hf_p16"])
def test_golden_transformers_crosscheck(golden_dir, name):
    import vdr
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg = vo.VitCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]))
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = vo.make_images(cfg, int(g["batch"]), seed=int(g["xseed"]))
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    got = hc.engine(cfg, w).forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity(got, torch.from_numpy(g["tokens"]), name, gate_l2(cfg.layers), emu["tokens"])


def test_reference_boundary_protocol():
    """R1/R2: load_model(...).model_name, .patch_embed(x) -> [B,n,D], .image_encoder(x) -> [B,D,h,w],
    get_dense_descriptor(model, img) -> (h,w,D) numpy — as tfds_dense_descriptor.py:110-139 uses them;
    torch.cuda.empty_cache() between calls (reference :137) must not break the engine."""
    import vdr
    cfg = vo.CONFIGS["vit_tiny16_224"]
    w = vo.make_weights(cfg, seed=2)
    model = vdr.load_model("vit_tiny16_224", weights=w)
    assert model.model_name == "vit_tiny16_224"
    x = vo.make_images(cfg, 2, seed=9)
    ref = vo.forward_images(cfg, w, x)
    pe = model.patch_embed(x.cuda())
    assert pe.shape == (2, 196, 192) and pe.is_cuda
    torch.cuda.empty_cache()
    enc = model.image_encoder(x.cuda())
    assert enc.shape == (2, 192, 14, 14)
    model.model_name = "dinov2"   # the reference assigns the attribute after construction
    f = vdr.get_dense_descriptor(model, x[0].numpy())
    assert f.shape == (14, 14, 192) and f.dtype == np.float32
    assert rel_l2(torch.from_numpy(f).reshape(196, 192), ref["patch_embed"][0]) < 1e-2
    model.model_name = "medsam"
    f2 = vdr.get_dense_descriptor(model, x[0].numpy())
    assert f2.shape == (14, 14, 192)
    assert rel_l2(torch.from_numpy(f2).reshape(196, 192), ref["dense"][0]) < 2e-2
    d = vdr.extract_dense(model, x.cuda())
    assert d.shape == (2, 14, 14, 192)
    np.testing.assert_array_equal(d[0], f2)
    with pytest.raises(ValueError):
        model.patch_embed(torch.zeros(1, 3, 100, 100).cuda())
    with pytest.raises(KeyError):
        vdr.load_model("vit_tiny16_224", weights={k: v for k, v in w.items() if k != "norm.bias"})
    # forward_into (the all-gather path) validates instead of converting: wrong dtype / size / layout are errors
    eng = model.engine
    xin = x.cuda()
    with pytest.raises(TypeError):
        eng.forward_into(xin.double(), torch.empty(2, 192, device="cuda"))
    with pytest.raises(ValueError):
        eng.forward_into(xin, torch.empty(1, 192, device="cuda"))            # too small: would be an OOB write
    with pytest.raises(ValueError):
        eng.forward_into(xin, torch.empty(2, 384, device="cuda")[:, ::2])    # not contiguous
    ok = eng.forward_into(xin, torch.empty(2, 192, device="cuda"))
    assert torch.equal(ok, eng.forward(xin, vdr.OUT_CLS))


def test_get_dense_descriptor_takes_the_raw_slice():
    """tfds_dense_descriptor.py:110-139: `get_dense_descriptor(model, img)` is called with the RAW slice -- (h, w) gray or
    (h, w, 3) colour in [0, 1] -- and runs `prepare_image` itself (gray2rgb + resize to 1024^2, resize to 896^2 for colour).
    The drop-in must do the same: equal to prepare_image -> encoder / patch_embed -> (h, w, D), bit for bit, and still take
    an already prepared (3, S, S) image."""
    import vdr
    from vdr import prep
    g = torch.Generator().manual_seed(21)
    # colour slice -> 896^2 -> the reference's 'dinov2' mode (patch embedding only)
    cfg = vo.VitCfg(896, 14, 3, 64, 1, 0, 128, pre_ln=False, has_cls=False, has_pos=False)
    w = vo.make_weights(cfg, seed=4)
    vc = vdr.VdrConfig(img=896, patch=14, dim=64, heads=1, layers=0, mlp_hidden=128, pre_ln=False, has_cls=False, has_pos=False)
    model = vdr.VitDescriptorModel(vc, w, "dinov2")
    rgb = torch.rand(150, 201, 3, generator=g).numpy()
    f = vdr.get_dense_descriptor(model, rgb)
    assert f.shape == (64, 64, 64) and f.dtype == np.float32
    x = prep.prepare_image(rgb)
    assert x.shape == (1, 3, 896, 896)
    want = model.patch_embed(x).cpu().numpy()[0].reshape(64, 64, 64)
    np.testing.assert_array_equal(f, want)
    np.testing.assert_array_equal(vdr.get_dense_descriptor(model, x[0].cpu().numpy()), want)  # prepared (3, S, S) as before
    with pytest.raises(ValueError):
        vdr.get_dense_descriptor(model, rgb[:, :, 0])  # a gray slice prepares to 1024^2: not this model's input
    # gray slice -> gray2rgb -> 1024^2 -> the reference's 'medsam' mode (image_encoder, [1, C, h, w] -> (h, w, C))
    cfg2 = vo.VitCfg(1024, 64, 3, 64, 1, 1, 128)
    w2 = vo.make_weights(cfg2, seed=5)
    vc2 = vdr.VdrConfig(img=1024, patch=64, dim=64, heads=1, layers=1, mlp_hidden=128)
    m2 = vdr.VitDescriptorModel(vc2, w2, "medsam")
    gray = torch.rand(300, 260, generator=g).numpy()
    f2 = vdr.get_dense_descriptor(m2, gray)
    assert f2.shape == (16, 16, 64)
    x2 = prep.prepare_image(gray)
    assert x2.shape == (1, 3, 1024, 1024)
    want2 = np.transpose(m2.image_encoder(x2).cpu().numpy()[0], (1, 2, 0))
    np.testing.assert_array_equal(f2, want2)
    ref = vo.forward_images(cfg2, w2, x2.cpu())["dense"][0].reshape(16, 16, 64)
    assert rel_l2(torch.from_numpy(f2), ref) < 2e-2


def test_dinov2_reference_mode_loads_a_real_checkpoint_layout():
    """The reference's 'dinov2' mode (tfds_dense_descriptor.py:70-90, 128-133): torch.hub dinov2_vits14, of which only
    `model.patch_embed(x)` runs, at 896^2.  A state_dict with that checkpoint's REAL key set and shapes (random values;
    pos_embed is [1, 1370, 384] = 518^2 / 14 + cls, which no 896^2 token model could take as it is) must load, and
    patch_embed must equal F.conv2d(stride 14) -> flatten -> transpose on the same bf16-rounded operands."""
    import vdr
    g = torch.Generator().manual_seed(5)
    D, L, F = 384, 12, 1536
    sd = {"cls_token": torch.randn(1, 1, D, generator=g), "pos_embed": torch.randn(1, 1370, D, generator=g) * 0.02,
          "mask_token": torch.zeros(1, D), "patch_embed.proj.weight": torch.randn(D, 3, 14, 14, generator=g) * 0.05,
          "patch_embed.proj.bias": torch.randn(D, generator=g) * 0.1, "norm.weight": torch.ones(D), "norm.bias": torch.zeros(D)}
    for i in range(L):
        p = f"blocks.{i}."
        sd.update({p + "norm1.weight": torch.ones(D), p + "norm1.bias": torch.zeros(D), p + "attn.qkv.weight": torch.zeros(3 * D, D),
                   p + "attn.qkv.bias": torch.zeros(3 * D), p + "attn.proj.weight": torch.zeros(D, D), p + "attn.proj.bias": torch.zeros(D),
                   p + "ls1.gamma": torch.ones(D), p + "norm2.weight": torch.ones(D), p + "norm2.bias": torch.zeros(D),
                   p + "mlp.fc1.weight": torch.zeros(F, D), p + "mlp.fc1.bias": torch.zeros(F), p + "mlp.fc2.weight": torch.zeros(D, F),
                   p + "mlp.fc2.bias": torch.zeros(D), p + "ls2.gamma": torch.ones(D)})
    model = vdr.load_model("dinov2", weights=sd)
    assert model.model_name == "dinov2" and model.cfg.img == 896 and model.cfg.patch == 14
    x = torch.rand(1, 3, 896, 896, generator=g)
    pe = model.patch_embed(x.cuda())                       # tfds_dense_descriptor.py:128
    assert pe.shape == (1, 4096, D) and pe.dtype == torch.float32
    ref = torch.nn.functional.conv2d(x.bfloat16().float(), sd["patch_embed.proj.weight"].bfloat16().float(),
                                     sd["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
    assert rel_l2(pe.cpu(), ref) < 4e-3
    f = vdr.get_dense_descriptor(model, x[0].numpy())      # :110-139 -> (64, 64, 384) float32
    assert f.shape == (64, 64, D) and f.dtype == np.float32
    np.testing.assert_array_equal(f.reshape(4096, D), pe[0].cpu().numpy())
    with pytest.raises(vdr.VdrError):                      # there is no CLS path in this mode, as in the reference
        model.forward_features(x.cuda())


def test_full_batch_properties_at_baseline_size():
    """Size-independent properties at BASELINE config-2 size (B=256 would need minutes of CPU oracle):
    (i) batch-permutation equivariance, (ii) duplicate images give bitwise-identical rows,
    (iii) a B=256 run agrees row-for-row with B=3 runs of the same images."""
    import vdr
    cfg = vo.CONFIGS["vit_base16_224"]
    w = vo.make_weights(cfg, seed=1)
    e = hc.engine(cfg, w)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(256, 3, 224, 224, generator=g).to(torch.bfloat16).cuda()
    x[17] = x[3]
    out = e.forward(x, vdr.OUT_CLS)
    assert out.shape == (256, 768) and torch.isfinite(out).all()
    assert torch.equal(out[17], out[3])
    perm = torch.randperm(256, generator=g).cuda()
    out_p = e.forward(x[perm], vdr.OUT_CLS)
    assert torch.equal(out_p, out[perm])
    small = e.forward(x[100:103], vdr.OUT_CLS)
    assert torch.equal(small, out[100:103])
    # the LayerNorm statistics finalised inside the persistent residual GEMMs (1182 tiles on 512 workgroups, three tile
    # columns per block of rows) instead of by their own launches: the same bits
    assert torch.equal(hc.engine(cfg, w, ln_fin_fused=True).forward(x, vdr.OUT_CLS), out)
    # The qkv linears of these launches run on tile variant 31 (csrc/gemm_8p.hip: 256-row tiles, one workgroup per CU), those
    # of the 3-image run on the ring4 tiles: the comparison above is 8-phase == ring4 bit for bit, LayerNorm fold included.
    # A batch whose token count is NOT a multiple of 256 (100 images = 19700 rows: 693 tiles, the last row tile 244 rows):
    # the kernel reads the workspace's padding rows behind row M and stores none of them -- every token, fold on and off.
    for fold in (True, False):
        ef = hc.engine(cfg, w, ln_fold=fold)
        big = ef.forward(x[:100].contiguous(), vdr.OUT_TOKENS)
        assert torch.isfinite(big.float()).all()
        for lo in (0, 47, 97):
            assert torch.equal(ef.forward(x[lo:lo + 3].contiguous(), vdr.OUT_TOKENS), big[lo:lo + 3]), (fold, lo)


@pytest.mark.parametrize("name,batch", [("p16_d128", 5), ("p14_d192", 3), ("dinov2_swiglu_ls", 4), ("vit_base16_224", 40),
                                        ("vit_base16_224", 100)])
@pytest.mark.parametrize("resid_fp32", [False, True])
def test_layernorm_statistics_finalised_inside_the_residual_gemm(name, batch, resid_fp32):
    """vdr_config.ln_fin_fused = 1: the workgroup of the out-projection / fc2 GEMM that adds the LAST partial
    sums to a block of rows turns them into (mean, rstd) itself (csrc/gemm_kernels.h finalize_rows_if_last: agent-scope
    stores and loads of the partials, one counter per block of tile rows) -- no ln_finalize launch between a residual GEMM
    and the qkv / fc1 that folds LayerNorm (norm1 / norm2 of the frozen ViTs called at tfds_dense_descriptor.py:123).  Same
    arithmetic as the separate launch (the default): every output bit for bit, small launches (128 x 128 ring4 tiles, a handful of
    workgroups) and large ones (persistent 128 x 256 tiles on every CU, three tile columns per block of rows racing for
    the counter; ViT-B at 40 / 100 images), CLS tail and full last block, run twice (the counters must come back to zero)."""
    import vdr
    cfg = SMALL[name] if name in SMALL else vo.CONFIGS[name]
    w = vo.make_weights(cfg, seed=71, scale=0.05) if name in SMALL else vo.make_weights(cfg, seed=71)
    g = torch.Generator().manual_seed(72)
    x = torch.rand(batch, cfg.in_chans, cfg.img, cfg.img, generator=g).to(torch.bfloat16).cuda()
    for full in (False, True):
        a = hc.engine(cfg, w, resid_fp32=resid_fp32, full_last_block=full, ln_fin_fused=True)
        b = hc.engine(cfg, w, resid_fp32=resid_fp32, full_last_block=full)
        for mode in (vdr.OUT_CLS, vdr.OUT_TOKENS):
            want = b.forward(x, mode)
            assert torch.isfinite(want.float()).all()
            for rep in range(2):
                assert torch.equal(a.forward(x, mode), want), (name, full, mode, rep)
    if name == "vit_base16_224" and batch == 100:
        # the profiler sees the difference (launches large enough for the 8-phase qkv / fc1, which read finalised statistics):
        # one ln_finalize launch per forward -- the statistics of the assembled tokens -- instead of two per block
        counts = []
        for e in (hc.engine(cfg, w, resid_fp32=resid_fp32, ln_fin_fused=True), hc.engine(cfg, w, resid_fp32=resid_fp32)):
            e.profile(True)
            e.forward(x, vdr.OUT_TOKENS)
            counts.append(e.profile_read().get("layernorm", {}).get("launches", 0))
            e.profile(False)
        assert counts == [1, 2 * cfg.layers], counts


# ---- SAM / MedSAM image encoder (the reference's default backbone) ----------------
@pytest.mark.parametrize("name,cfgargs,batch", [
    ("grid10_win4_padded", dict(img=160, patch=16, dim=64, heads=1, layers=3, mlp_hidden=128, window=4, global_idx=(1,), out_chans=64), 3),
    ("grid14_win7", dict(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64), 2),
    ("grid14_win4_allwindow", dict(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=4, global_idx=(), out_chans=128), 2),
])
def test_sam_encoder_small(name, cfgargs, batch):
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(**cfgargs)
    w = so.make_weights(cfg, seed=21, scale=0.05)
    x = so.make_images(cfg, batch, seed=22)
    ref = so.sam_forward(cfg, w, x)
    emu = so.sam_forward(cfg, w, x, emulate_bf16=True)
    e = hc.sam_engine(cfg, w)
    tok = e.forward(x.cuda(), vdr.OUT_TOKENS)
    g = cfg.grid
    check_parity(tok, ref["tokens"].reshape(batch, g * g, cfg.dim), f"sam {name} tokens", gate_l2(cfg.layers),
                 emu["tokens"].reshape(batch, g * g, cfg.dim))
    out = e.forward(x.cuda(), vdr.OUT_ENCODER)  # [B, g, g, C] channel-last
    assert out.shape == (batch, g, g, cfg.out_chans)
    check_parity(out, ref["out"].permute(0, 2, 3, 1), f"sam {name} neck output", gate_l2(cfg.layers) + 4e-3,
                 emu["out"].permute(0, 2, 3, 1))


@pytest.mark.parametrize("cfgargs,batch", [
    (dict(img=160, patch=16, dim=64, heads=1, layers=3, mlp_hidden=128, window=4, global_idx=(1,), out_chans=64), 3),
    (dict(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64), 2),
])
def test_sam_encoder_fp8(cfgargs, batch):
    """fp8 (qkv / fc1 / fc2 as MX-fp8) on the SAM encoder: LayerNorm -> MX in window-partition order with zero
    padding rows, the un-partitioning out-projection stays bf16."""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(**cfgargs)
    w = so.make_weights(cfg, seed=21, scale=0.05)
    x = so.make_images(cfg, batch, seed=22)
    ref = so.sam_forward(cfg, w, x)
    emx = so.sam_forward(cfg, w, x, emulate_bf16="mx")
    e = hc.sam_engine(cfg, w, fp8=1)
    g = cfg.grid
    tok = e.forward(x.cuda(), vdr.OUT_TOKENS)
    check_parity_fp8(tok, ref["tokens"].reshape(batch, g * g, cfg.dim), emx["tokens"].reshape(batch, g * g, cfg.dim),
                     cfg.layers, "sam fp8 tokens")
    out = e.forward(x.cuda(), vdr.OUT_ENCODER)
    check_parity_fp8(out, ref["out"].permute(0, 2, 3, 1), emx["out"].permute(0, 2, 3, 1), cfg.layers, "sam fp8 neck output")
    assert torch.equal(out, e.forward(x.cuda(), vdr.OUT_ENCODER))


def test_sam_golden_transformers_crosscheck(golden_dir):
    import vdr
    from oracle import sam_oracle as so
    g = np.load(os.path.join(golden_dir, "sam_hf_w7.npz"), allow_pickle=False)
    cfg = so.SamCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]),
                    int(g["window"]), tuple(int(i) for i in g["global_idx"]), int(g["out_chans"]), 1e-6)
    w = so.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = so.make_images(cfg, int(g["batch"]), seed=int(g["xseed"]))
    out = hc.sam_engine(cfg, w).forward(x.cuda(), vdr.OUT_ENCODER).permute(0, 3, 1, 2)
    want = torch.from_numpy(g["out"])
    assert rel_l2(out.cpu(), want) <= gate_l2(cfg.layers) + 4e-3
    assert min_cos(out.cpu().permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)) >= 0.999


def test_medsam_vit_b_1024_geometry_and_boundary():
    """The reference's default path (tfds_dense_descriptor.py:93-126): load_model('medsam', path) ->
    model.image_encoder(x[1,3,1024,1024]) -> [1,256,64,64] -> (64,64,256) numpy.  Full SAM ViT-B geometry
    (768/12 heads, window 14 -> 25 zero-padded windows, global attention over 4096 tokens) with the depth cut
    to 3 blocks (window, window, global) so the CPU oracle stays in seconds."""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(layers=3, global_idx=(2,))
    w = so.make_weights(cfg, seed=23)
    x = so.make_images(cfg, 1, seed=24)
    ref = so.sam_forward(cfg, w, x)
    vc = vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "layers": 3, "global_blocks": (2,)})
    model = vdr.VitDescriptorModel(vc, w, "medsam")
    enc = model.image_encoder(x.cuda())
    assert enc.shape == (1, 256, 64, 64)
    assert rel_l2(enc.cpu(), ref["out"]) <= gate_l2(3) + 4e-3
    assert min_cos(enc.cpu().permute(0, 2, 3, 1), ref["out"].permute(0, 2, 3, 1)) >= 0.999
    f = vdr.get_dense_descriptor(model, x[0].numpy())
    assert f.shape == (64, 64, 256) and f.dtype == np.float32
    np.testing.assert_array_equal(f, np.transpose(enc[0].cpu().numpy(), (1, 2, 0)))
    # segment_anything checkpoint key names are accepted as they are
    from vdr.model import from_sam_state_dict
    sam_sd = {("image_encoder." + k).replace(".mlp.fc1.", ".mlp.lin1.").replace(".mlp.fc2.", ".mlp.lin2."): v for k, v in w.items()}
    sam_sd["prompt_encoder.dummy"] = torch.zeros(1)
    assert sorted(from_sam_state_dict(sam_sd)) == sorted(w)


@pytest.mark.parametrize("fp8", [0, 1])
def test_batch_size_sweep_rows_do_not_depend_on_the_batch(fp8):
    """Odd batch sizes (1, 2, 3, 5, 17, 65) on a small ViT, bf16 and fp8: every image's CLS / dense rows are bitwise
    what the same image gives in any other batch (edge tiles of every GEMM shape, ragged attention launches)."""
    import vdr
    cfg = SMALL["p14_d192"]
    w = vo.make_weights(cfg, seed=5, scale=0.05)
    e = hc.engine(cfg, w, fp8=fp8)
    x = vo.make_images(cfg, 65, seed=6).cuda()
    full_cls = e.forward(x, vdr.OUT_CLS)
    full_dense = e.forward(x, vdr.OUT_DENSE)
    for B in (1, 2, 3, 5, 17):
        sel = torch.arange(B) * 3 % 65
        assert torch.equal(e.forward(x[sel], vdr.OUT_CLS), full_cls[sel]), B
        assert torch.equal(e.forward(x[sel], vdr.OUT_DENSE), full_dense[sel]), B


@pytest.mark.parametrize("tag", ["tiny", "refdim"])
def test_golden_reference_bimodal_classifier(golden_dir, tag):
    """models_archs.TransformerNoduleBimodalClassifier (:38-124) golden vectors made by the reference itself: the
    drop-in class with the reference's state_dict keys, CT + PET (cross attention), CT only, PET only."""
    import vdr
    from oracle import bimodal_oracle as bo
    g = np.load(os.path.join(golden_dir, f"bimodal_{tag}.npz"), allow_pickle=False)
    dim, lc, lp = int(g["dim"]), int(g["layers_ct"]), int(g["layers_pet"])
    rc, rp, hc, hp, ncls = float(g["ratio_ct"]), float(g["ratio_pet"]), int(g["heads_ct"]), int(g["heads_pet"]), int(g["classes"])
    sd = bo.make_state_dict(dim, int(rc * dim), int(rp * dim), lc, lp, ncls, seed=int(g["seed"]))
    m = vdr.TransformerNoduleBimodalClassifier(dim, rc, rp, hc, hp, lc, lp, ncls)  # reference signature (models_archs.py:39-43)
    m.load_state_dict(sd)                                                          # models_archs.py:32-35
    x_ct, x_pet = torch.from_numpy(g["x_ct"]).cuda(), torch.from_numpy(g["x_pet"]).cuda()
    L = max(lc, lp) + 1  # encoder depth + the cross-attention / fusion stage
    for mode, (a, b) in (("both", (x_ct, x_pet)), ("ct", (x_ct, None)), ("pet", (None, x_pet))):
        out = m(a, b)
        assert len(out) == 4
        for name, o in zip(("logits_petct", "cls_petct", "logits_ct", "logits_pet"), out):
            want = torch.from_numpy(g[f"{mode}_{name}"])
            assert o.shape == want.shape and o.dtype == torch.float32 and o.is_cuda, (mode, name)
            if name.startswith("cls"):
                r, c = rel_l2(o.cpu(), want), min_cos(o.cpu(), want)
                print(f"bimodal_{tag} {mode} {name}: relL2 {r:.3e} min cos {c:.6f}")
                assert r <= gate_l2(L) and c >= 0.999, (mode, name, r, c)
            else:
                err = (o.cpu() - want).abs().max().item()
                assert err < 3e-2, (mode, name, err)
    with pytest.raises(AssertionError):
        m(None, None)
    # single-modality mode returns the encoder's CLS row: identical to the unimodal engine path
    assert torch.equal(m(x_ct, None)[1], m.engines["ct"].forward_tokens(x_ct, vdr.OUT_CLS))


@pytest.mark.parametrize("name", ["p16_d128", "p14_d192", "dinov2_swiglu_ls"])
@pytest.mark.parametrize("ln_fold", [True, False])
def test_resid_fp32_master_copy_of_the_residual_stream(name, ln_fold):
    """vdr_config.resid_fp32: the out-projection / fc2 epilogues keep an fp32 master copy of the residual stream (the
    reference computes in fp32 throughout, tfds_dense_descriptor.py:123); LayerNorm / the final norm read it, the next GEMM
    multiplies its bf16 rounding.  (i) closer to the fp32 oracle than the bf16 stream, and as close to the emulating oracle
    run with vo.RESID_FP32 as the bf16 path is to its emulation; (ii) the CLS tail of the last block stays bitwise the full
    block; (iii) micro-batches do not change a row."""
    import vdr
    cfg = SMALL[name]
    w = vo.make_weights(cfg, seed=61, scale=0.05)
    x = vo.make_images(cfg, 5, seed=62)
    ref = vo.forward_images(cfg, w, x)
    vo.RESID_FP32 = True
    try:
        emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    finally:
        vo.RESID_FP32 = False
    e32 = hc.engine(cfg, w, ln_fold=ln_fold, resid_fp32=True)
    e16 = hc.engine(cfg, w, ln_fold=ln_fold)
    tok32 = e32.forward(x.cuda(), vdr.OUT_TOKENS).float().cpu()
    tok16 = e16.forward(x.cuda(), vdr.OUT_TOKENS).float().cpu()
    r32, r16, remu = rel_l2(tok32, ref["tokens"]), rel_l2(tok16, ref["tokens"]), rel_l2(tok32, emu["tokens"])
    print(f"{name} fold={ln_fold}: relL2 vs fp32 oracle: bf16 stream {r16:.3e}, fp32 stream {r32:.3e}; fp32 stream vs its emulation {remu:.3e}")
    assert torch.isfinite(tok32).all() and not torch.equal(tok32, tok16)
    assert r32 <= gate_l2(cfg.layers) and r32 <= 1.05 * r16 and min_cos(tok32, ref["tokens"]) >= 0.999
    assert remu <= gate_l2(cfg.layers)
    full = hc.engine(cfg, w, ln_fold=ln_fold, resid_fp32=True, full_last_block=True)
    ref_cls = full.forward(x.cuda(), vdr.OUT_CLS)
    assert torch.equal(ref_cls, full.forward(x.cuda(), vdr.OUT_TOKENS)[:, 0])
    for mb in (0, 2):
        got = hc.engine(cfg, w, ln_fold=ln_fold, resid_fp32=True, micro_batch=mb).forward(x.cuda(), vdr.OUT_CLS)
        assert torch.equal(got, ref_cls), f"micro_batch {mb}"
    assert torch.equal(e32.forward(x.cuda(), vdr.OUT_DENSE), full.forward(x.cuda(), vdr.OUT_DENSE))


def test_bench_plain_run_dumps_the_features_of_its_last_timed_step(tmp_path):
    """A plain `bench.py` run: one JSON line with the headline keys and none of the --full figures, `steps` as asked, and
    --dump-outputs holding what the timed path returned -- bitwise the same forward on bench.py's seeded inputs."""
    import json
    import subprocess
    import sys
    import vdr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert line["steps"] == 3 and line["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0
    assert not {"kernels", "roofline", "full_last_block", "cpu_baseline"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["cls_features.npy"]
    got = np.load(tmp_path / "cls_features.npy")
    ocfg = vo.CONFIGS["vit_base16_224"]
    assert got.dtype == np.float32 and got.shape == (8, ocfg.dim)
    model = vdr.load_model("vit_base16_224", weights=vo.make_weights(ocfg, seed=1), device=torch.device("cuda", 0))
    images = torch.rand(8, 3, ocfg.img, ocfg.img, generator=torch.Generator().manual_seed(1000)).to(torch.bfloat16).cuda()
    want = torch.empty(8, ocfg.dim, device="cuda")
    model.engine.forward_into(images, want, vdr.OUT_CLS)
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy())
