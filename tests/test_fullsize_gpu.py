"""GPU: BASELINE configs 4 and 5 and the reference's default backbone at FULL depth and at the full per-GPU batch.

The per-geometry tests in test_model_gpu.py cut the depth to 2-3 blocks so the CPU oracle stays in seconds; rounding
error accumulates over depth (the gate 4e-3 + 3e-3 sqrt(L) models exactly that), so here every model runs all of its
blocks: (i) against the fp32 oracle at batch 1-2 (tens of seconds of CPU), (ii) at the per-GPU batch of the BASELINE
config (64 dense / 32 fp8) through size-independent properties: duplicate images give bitwise equal rows, a batch
permutation permutes the rows, and a row does not depend on the batch it travels in.

  config 4  ViT-L/14 336^2 bf16, 24 blocks, dense per-patch descriptors (tfds_dense_descriptor.py:130-133 contract)
  config 5  DINOv2 ViT-g/14 224^2, 40 blocks, SwiGLU + LayerScale, bf16 and MX-fp8 weights (fp8 = 1)
  MedSAM    SAM ViT-B image encoder, 12 blocks at 1024^2 (tfds_dense_descriptor.py:93-107, 122-126)
"""
import pytest
import torch

from model_gates import (check_batch_properties, check_parity, gate_l2, gate_l2_fp8, inject_outlier_channels, min_cos,
                         rel_l2)
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


def test_config4_vit_large14_336_full_depth_and_full_batch():
    import vdr
    cfg = vo.CONFIGS["vit_large14_336"]
    assert cfg.layers == 24 and cfg.n_tokens == 577
    w = vo.make_weights(cfg, seed=4)
    x = vo.make_images(cfg, 2, seed=5)
    ref = vo.forward_images(cfg, w, x)
    m = vdr.load_model("vit_large14_336", weights=w)
    e = m.engine
    xd = x.cuda().to(torch.bfloat16)
    dense = e.forward(xd, vdr.OUT_DENSE, torch.bfloat16)          # config 4's output: [B, 576, 1024] bf16
    assert dense.shape == (2, 576, 1024) and dense.dtype == torch.bfloat16
    check_parity(dense, ref["dense"], "ViT-L/14@336 L=24 dense (bf16 out)", gate_l2(24) + 2e-3)  # + the output rounding
    check_parity(e.forward(xd, vdr.OUT_CLS), ref["cls"], "ViT-L/14@336 L=24 cls", gate_l2(24))
    # full per-GPU batch of config 4 (512 / 8 GPUs = 64 images)
    g = torch.Generator().manual_seed(1)
    xb = torch.rand(64, 3, cfg.img, cfg.img, generator=g).to(torch.bfloat16).cuda()
    xb[63] = xb[1]
    out = check_batch_properties(lambda t: e.forward(t, vdr.OUT_DENSE, torch.bfloat16), xb)
    assert out.shape == (64, 576, 1024)


@pytest.mark.parametrize("fp8", [0, 1])
def test_config5_dinov2_giant14_full_depth_and_full_batch(fp8):
    """fp8 = 1 is BASELINE config 5 ("DINOv2 ViT-g/14 fp8 weights (CDNA4 fp8 MFMA)"); gates as in test_model_gpu.py:
    per-row cosine >= 0.99 against the reference's fp32 arithmetic and rel L2 <= 4e-2 + 4e-2 sqrt(L)."""
    import vdr
    cfg = vo.CONFIGS["dinov2_giant14_224"]
    assert cfg.layers == 40 and cfg.n_tokens == 257
    w = vo.make_weights(cfg, seed=1)
    x = vo.make_images(cfg, 2, seed=3)
    ref = vo.forward_images(cfg, w, x)
    m = vdr.load_model("dinov2_giant14_224", weights=w, fp8=fp8)
    e = m.engine
    gate, cos = (gate_l2_fp8(40), 0.99) if fp8 else (gate_l2(40), 0.999)
    tag = "MX-fp8 weights" if fp8 else "bf16"
    check_parity(e.forward(x.cuda(), vdr.OUT_CLS), ref["cls"], f"DINOv2 ViT-g/14 L=40 {tag} cls", gate, cos=cos)
    check_parity(e.forward(x.cuda(), vdr.OUT_DENSE), ref["dense"], f"DINOv2 ViT-g/14 L=40 {tag} dense", gate, cos=cos)
    # full per-GPU batch of config 5 (256 / 8 GPUs = 32 images)
    g = torch.Generator().manual_seed(2)
    xb = torch.rand(32, 3, cfg.img, cfg.img, generator=g).to(torch.bfloat16).cuda()
    xb[31] = xb[1]
    out = check_batch_properties(lambda t: e.forward(t, vdr.OUT_CLS, torch.float32), xb)
    assert out.shape == (32, 1536)


@pytest.mark.parametrize("fp8", [0, 1])
def test_medsam_vit_b_1024_all_twelve_blocks(fp8):
    """The reference's default backbone as it runs it: one 1024^2 slice through the whole SAM ViT-B image encoder
    (12 blocks, windows of 14 + global blocks 2 / 5 / 8 / 11, rel-pos, neck) against oracle/sam_oracle.py."""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SAM_VIT_B
    assert cfg.layers == 12 and cfg.img == 1024
    w = so.make_weights(cfg, seed=1)
    x = so.make_images(cfg, 1, seed=3)
    ref = so.sam_forward(cfg, w, x)["out"].permute(0, 2, 3, 1)    # (1, 64, 64, 256): the layout get_dense_descriptor returns
    m = vdr.load_model("medsam", weights=w, fp8=fp8)
    got = m.engine.forward(x.cuda(), vdr.OUT_ENCODER, torch.float32)
    assert got.shape == (1, 64, 64, 256)
    if fp8:
        check_parity(got, ref, "MedSAM 1024^2 L=12 MX-fp8 neck output", gate_l2_fp8(12), cos=0.99)
    else:
        # the neck ends in a LayerNorm2d over 256 channels, which re-normalises the accumulated error: same gate
        check_parity(got, ref, "MedSAM 1024^2 L=12 neck output", gate_l2(12))
    # batch of slices (what vdr.pipeline.generate_features feeds): rows do not depend on the batch
    xb = torch.cat([x, so.make_images(cfg, 2, seed=4)]).cuda()
    outb = m.engine.forward(xb, vdr.OUT_ENCODER, torch.float32)
    assert torch.equal(outb[0], got[0])


def test_config5_massive_activation_channels_at_full_depth():
    """The outlier-channel injection of test_model_gpu.py (LayerNorm gains x30-100, residual channels at +300 / -120 in every
    patch token: what DINOv2-g checkpoints carry and seeded Gaussian weights do not) at the FULL depth of config 5.
    bf16 stays at its usual gate.  MX-fp8 with every row quantised loses the CLS rows (their value is their own MX-fp8 MLP
    chain, 40 blocks deep: emulating oracle 0.919, tools/fp8_outlier_analysis.py); with vdr_config.fp8_cls_bf16 -- the CLS
    rows' MLP on the bf16 weights -- they come back to 0.989 (emulation), gated here at 0.985: the CLS feature IS config
    5's output, so that switch is what `bench.py --fp8 --fp8-cls-bf16` times and what a massive-activation checkpoint
    should be loaded with.  Patch rows are dominated by the injected channels (cosine ~ 1 by construction)."""
    import vdr
    cfg = vo.CONFIGS["dinov2_giant14_224"]
    w, _ = inject_outlier_channels(vo.make_weights(cfg, seed=31), cfg.layers, cfg.dim, 32, "mlp.w12")
    x = vo.make_images(cfg, 2, seed=33)
    ref = vo.forward_images(cfg, w, x)["cls"]

    def cls_of(**kw):
        got = vdr.load_model("dinov2_giant14_224", weights=w, **kw).engine.forward(x.cuda(), vdr.OUT_CLS).float().cpu()
        assert torch.isfinite(got).all()
        return min_cos(got, ref), rel_l2(got, ref)

    c16, r16 = cls_of()
    c8, r8 = cls_of(fp8=1)
    c8c, r8c = cls_of(fp8=1, fp8_cls_bf16=True)
    print(f"ViT-g/14 L=40, injected massive channels, CLS rows vs fp32: bf16 cos {c16:.6f} relL2 {r16:.3e} | MX-fp8 cos {c8:.6f} relL2 {r8:.3e} "
          f"| MX-fp8 + fp8_cls_bf16 cos {c8c:.6f} relL2 {r8c:.3e}")
    assert c16 >= 0.999 and r16 <= 2 * gate_l2(40)   # (emulation: 0.99917, 3.9e-2 -- the CLS row carries twice the usual rel-L2 here)
    assert c8c >= 0.985 and c8c > c8 + 0.03          # the switch restores what the all-MX-fp8 path loses (emulation 0.9886 vs 0.9188)
    assert c8 >= 0.88                                 # documented, not endorsed: every row MX-fp8 under massive channels


@pytest.mark.parametrize("name,layers,gate", [("vit_large14_336", 24, 1e-2), ("dinov2_giant14_224", 40, 1.1e-2)])
def test_resid_fp32_brings_the_deep_configs_to_the_survey_gate(name, layers, gate):
    """SURVEY 8d states rel-L2 <= 1e-2 for the bf16 path against the fp32 oracle; with the residual stream stored as bf16 the
    rounding accumulates over the blocks (1.2e-2 at 24 blocks, 1.7e-2 at 40: test_config4 / test_config5 gate at
    4e-3 + 3e-3 sqrt(L) -- a stated deviation).  vdr_config.resid_fp32 keeps an fp32 master copy of the stream: ViT-L/14@336
    (config 4) is gated at the survey's 1e-2 with it; ViT-g/14 (config 5, bf16 variant) lands ON it (emulation
    tools/resid_precision.py: CLS 1.015e-2, dense 9.8e-3) and is gated at 1.1e-2."""
    import vdr
    cfg = vo.CONFIGS[name]
    assert cfg.layers == layers
    w = vo.make_weights(cfg, seed=1)
    x = vo.make_images(cfg, 2, seed=3)
    ref = vo.forward_images(cfg, w, x)
    e = vdr.load_model(name, weights=w, resid_fp32=True).engine
    xd = x.cuda().to(torch.bfloat16) if name == "vit_large14_336" else x.cuda()
    if name == "vit_large14_336":
        ref = vo.forward_images(cfg, w, xd.float().cpu())
    check_parity(e.forward(xd, vdr.OUT_CLS), ref["cls"], f"{name} L={layers} resid_fp32 cls", gate, cos=0.9995)
    check_parity(e.forward(xd, vdr.OUT_DENSE), ref["dense"], f"{name} L={layers} resid_fp32 dense (fp32 out)", gate, cos=0.9995)
