"""CPU: SAM's box-prompt encoder and mask decoder without a device -- the float64 restatement (tests/sam_decoder_ref.py)
against the transformers.SamModel goldens, the table of the two key spellings, what load_model keeps of a checkpoint, every
refusal of the Python calls, the C entry points (declared, bound, exported, refusing bad arguments before the device check)
and the box scaling of segment_slice."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sam_decoder_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")


@pytest.fixture(scope="module")
def cases(golden_dir):
    return {tag: R.golden_case(golden_dir, tag) for tag in ("g8", "g10")}   # (checks the SHA-256 of the drawn weights first)


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_restatement_reproduces_the_transformers_golden(cases, tag):
    """gate: 4 x the difference measured when the golden was made (README_sam_decoder.md; fp32 sums of the torch module
    reorder between BLAS builds), and the bf16-rounding mode reproduces its stored difference likewise"""
    c = cases[tag]
    assert tuple(c["boxes"].shape) == {"g8": (2, 1, 4), "g10": (1, 3, 4)}[tag]
    lg, iou = R.decode(c["weights"], c["emb"], c["boxes"], c["cfg"], "f64")
    got = R.diffs(lg, iou, c["all4"], c["iou4"])
    print(f"{tag}: f64 restatement vs golden relL2 {got[0]:.3e} max|d| {got[1]:.3e} iou {got[2]:.3e}  (stored {c['f64_diff']})")
    for v, stored in zip(got, c["f64_diff"]):
        assert v <= 4.0 * stored
    assert c["f64_diff"][0] < 1e-5   # the definition itself: fp32 noise of the golden, nothing structural
    lg, iou = R.decode(c["weights"], c["emb"], c["boxes"], c["cfg"], "bf16")
    got = R.diffs(lg, iou, c["all4"], c["iou4"])
    for v, stored in zip(got, c["bf16_diff"]):
        assert v <= 2.0 * stored
    # the spread the mask test needs: fewer than 10 % of the golden's logits within the device gate of zero
    assert float((c["all4"].abs() < 2.0 * c["bf16_diff"][1]).double().mean()) < 0.10
    if tag == "g10":
        assert float(c["boxes"][0, 1, 0]) == float(c["boxes"][0, 1, 2])   # the degenerate box


def test_eps_matters_and_the_two_sets_are_told_apart(cases):
    """transformers applies layer_norm_eps = 1e-6 to the decoder's LayerNorms, segment_anything nn.LayerNorm's 1e-5"""
    import vdr
    assert vdr.segment.HF_EPS == R.HF_EPS and vdr.segment.SA_EPS == R.SA_EPS and R.HF_EPS != R.SA_EPS
    c = cases["g8"]
    assert c["eps"] == R.HF_EPS


def test_name_table_round_trips_both_spellings():
    from vdr.weights import sam_decoder_name, split_sam_decoder_weights
    w = R.draw_weights(3)
    assert sorted(w) == sorted(R.decoder_shapes(128))
    hf = R.to_hf(w)
    assert "mask_decoder.output_hypernetworks_mlps.2.proj_in.weight" in hf and "mask_decoder.upscale_conv2.bias" in hf
    assert "mask_decoder.transformer.layers.1.layer_norm4.weight" in hf and "prompt_encoder.point_embed.3.weight" in hf
    assert "shared_image_embedding.positional_embedding" in hf
    for k in w:
        assert sam_decoder_name(sam_decoder_name(k, "hf"), "sa") == k, k
    # the ambiguous spot: layers.0 is the first linear for segment_anything, the middle one for transformers
    assert sam_decoder_name("mask_decoder.iou_prediction_head.layers.0.weight", "hf") == "mask_decoder.iou_prediction_head.proj_in.weight"
    assert sam_decoder_name("mask_decoder.iou_prediction_head.layers.0.weight", "sa") == "mask_decoder.iou_prediction_head.layers.1.weight"
    for sd in (w, hf):
        rest, dec = split_sam_decoder_weights({**sd, "pos_embed": torch.zeros(1), "image_encoder.neck.0.weight": torch.zeros(1)})
        assert sorted(rest) == ["image_encoder.neck.0.weight", "pos_embed"] and sorted(dec) == sorted(w)
        assert all(torch.equal(dec[k], w[k]) for k in w)
    rest, dec = split_sam_decoder_weights({"pos_embed": torch.zeros(1)})
    assert dec is None and list(rest) == ["pos_embed"]
    with pytest.raises(ValueError):
        sam_decoder_name("x", "timm")


class _Cfg:
    window, img, patch = 14, 128, 16


class _Handle:
    """what the refusals look at, without an engine"""
    model_name = "medsam"
    device = "cpu"

    def __init__(self, window=14, decoder=True):
        self.cfg = _Cfg()
        self.cfg.window = window
        self.mask_decoder = type("D", (), {"g": 8})() if decoder else None
    has_mask_decoder = property(lambda self: self.mask_decoder is not None)


def test_python_calls_refuse_before_any_device_work():
    import vdr
    M = vdr.VitDescriptorModel
    x, emb, boxes = torch.zeros((1, 3, 128, 128)), torch.zeros((1, 256, 8, 8)), torch.zeros((1, 2, 4))
    for call in (lambda h: M.segment(h, x, boxes), lambda h: M.decode_masks(h, emb, boxes),
                 lambda h: vdr.segment_slice(h, np.zeros((20, 30), np.float32), [1, 2, 3, 4]),
                 lambda h: vdr.pipeline.segment_volume(h, np.zeros((20, 30, 2), np.float32), [1, 2, 3, 4])):
        with pytest.raises(ValueError, match="SAM / MedSAM model"):
            call(_Handle(window=0))                      # a model that is not SAM
        with pytest.raises(ValueError, match="encoder-only"):
            call(_Handle(decoder=False))                 # a SAM handle loaded without decoder weights
    h = _Handle()
    for bad in (torch.zeros((2, 4)), torch.zeros(4), torch.zeros((1, 2, 5)), torch.zeros((1, 0, 4)), torch.zeros((1, 2, 4), dtype=torch.bool),
                torch.zeros((1, 2, 4), dtype=torch.complex64), [[1, 2, 3, 4]], torch.zeros((2, 1, 4))):
        with pytest.raises(ValueError, match="boxes|box sets"):
            M.segment(h, x, bad)
        with pytest.raises(ValueError, match="boxes|box sets"):
            M.decode_masks(h, emb, bad)
    for bad in (torch.zeros((1, 256, 4, 4)), torch.zeros((1, 128, 8, 8)), torch.zeros((256, 8, 8)), torch.zeros((1, 256, 8, 10)), "emb"):
        with pytest.raises(ValueError, match="grid"):
            M.decode_masks(h, bad, boxes)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        M.segment(h, torch.zeros((3, 128, 128)), boxes)
    with pytest.raises(ValueError, match="slice"):
        vdr.segment_slice(h, np.zeros((4, 5, 2)), [1, 2, 3, 4])
    with pytest.raises(ValueError, match="box must be"):
        vdr.segment_slice(h, np.zeros((4, 5)), [1, 2, 3])
    with pytest.raises(ValueError, match="boxes must be"):
        vdr.pipeline.segment_volume(h, np.zeros((20, 30, 3), np.float32), np.zeros((2, 4)))
    with pytest.raises(ValueError, match="img_3d"):
        vdr.pipeline.segment_volume(h, np.zeros((20, 30), np.float32), [1, 2, 3, 4])
    # an encoder-only checkpoint: nothing of the decoder is asked for, load_model's split finds none
    from vdr.weights import split_sam_decoder_weights
    assert split_sam_decoder_weights({"image_encoder.pos_embed": torch.zeros(1)})[1] is None
    # the host refusals of the op wrappers
    from vdr import ops
    t = torch.zeros((7, 128), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="HIP device"):
        ops.cross_attention(t, t, t, 1, 7, 7, 8, 16)
    with pytest.raises(TypeError, match="HIP device"):
        ops.token_linear(t, t)
    with pytest.raises(ValueError, match="mask_upscale"):
        ops.mask_upscale(t, t, t, t, 1, 1)


def test_segment_slice_scales_the_box_by_the_resize_factors():
    """a 100 (h) x 250 (w) slice prepared at 1024^2: x by 1024 / 250 = 4.096, y by 1024 / 100 = 10.24"""
    from vdr.segment import scale_box
    assert scale_box((25, 10, 125, 50), 100, 250, 1024) == (25 * 4.096, 10 * 10.24, 125 * 4.096, 50 * 10.24)
    assert scale_box((25, 10, 125, 50), 100, 250, 1024) == (102.4, 102.4, 512.0, 512.0)
    assert scale_box((0, 0, 250, 100), 100, 250, 128) == (0.0, 0.0, 128.0, 128.0)
    sel = __import__("vdr").segment.select_masks
    lg, iou = torch.arange(2 * 3 * 4.0).reshape(2, 3, 4, 1, 1), torch.arange(24.0).reshape(2, 3, 4)
    assert torch.equal(sel(lg, iou, False)[0], lg[:, :, :1]) and torch.equal(sel(lg, iou, True)[1], iou[:, :, 1:])
    seg = __import__("vdr").Segmentation(torch.tensor([[[[[-1.0, 1.0], [1.0, 3.0]]]]]), torch.zeros((1, 1, 1)), (4, 4))
    assert tuple(seg.logits().shape) == (1, 1, 1, 4, 4) and seg.masks().dtype == torch.bool
    assert torch.equal(seg.logits(size=(2, 2)), seg.low_res_logits) and int(seg.masks(threshold=0.5).sum()) < 16


def test_header_binding_and_exports_declare_the_mask_decoder_ops():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    for name in ("vdr_op_cross_attention", "vdr_op_token_linear", "vdr_op_mask_upscale", "vdr_mask_decoder_create",
                 "vdr_mask_decoder_num_weights", "vdr_mask_decoder_set_weight", "vdr_mask_decoder_finalize", "vdr_mask_decoder_workspace_bytes",
                 "vdr_mask_decode"):
        assert re.search(r"\bint " + name + r"\(", src) and name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
    for name in ("vdr_mask_decoder_weight_name", "vdr_mask_decoder_destroy"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert C.sizeof(_lib.vdr_mask_decoder_config) == 4 * 14   # 11 int32 fields + 3 floats
    assert _lib.load().vdr_abi_version() == 8
    for name in ("cross_attention", "token_linear", "mask_upscale"):
        assert callable(getattr(ops, name))
    for name in ("segment", "decode_masks", "has_mask_decoder"):
        assert hasattr(vdr.VitDescriptorModel, name)
    assert callable(vdr.segment_slice) and callable(vdr.pipeline.segment_volume) and vdr.segment.MaskDecoder.LAUNCHES == 52
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^NOCONTRACT :=.*\bmask_decoder\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\bmask_decoder\.hip\b", mk, re.M)


def test_ops_refuse_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    q, k, v, out, tab = (base + 1024 * i for i in range(5))

    def xa(q=q, ldq=128, qa=None, k=k, ldk=384, ka=tab, v=v, ldv=384, out=out, ldo=128, P=2, tq=7, tk=100, H=8, dh=16):
        return lib.vdr_op_cross_attention(q, ldq, qa, k, ldk, ka, v, ldv, out, ldo, P, tq, tk, H, dh, None)
    for kw in (dict(dh=8), dict(dh=64), dict(dh=0), dict(tq=17, tk=17), dict(tq=100, tk=4096), dict(H=16, dh=32, ldq=512, ldk=512, ldv=512, ldo=512)):
        assert xa(**kw) == -7, kw   # VDR_ERR_UNSUPPORTED
        assert lib.vdr_last_error(None).startswith(b"vdr_op_cross_attention: ")
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(P=0), dict(P=70000), dict(tq=0), dict(tk=-1), dict(H=0),
               dict(ldq=120), dict(ldk=132), dict(ldv=64), dict(ldo=127), dict(q=q + 2), dict(k=k + 8), dict(ka=tab + 4), dict(out=out + 6)):
        assert xa(**kw) == -1, kw   # VDR_ERR_INVALID

    def tl(x=q, ldx=256, xadd=None, ldxa=0, W=k, b=tab, r=None, ldr=0, y=out, dt=1, ldy=128, M=7, N=128, K=256, groups=1, relu=0):
        return lib.vdr_op_token_linear(x, ldx, xadd, ldxa, W, b, r, ldr, y, dt, ldy, M, N, K, groups, relu, None)
    for kw in (dict(K=100, ldx=100), dict(K=4096, ldx=4096)):
        assert tl(**kw) == -7, kw
    for kw in (dict(x=None), dict(W=None), dict(y=None), dict(dt=2), dict(M=0), dict(N=0), dict(K=0), dict(groups=0), dict(groups=8),
               dict(relu=2), dict(ldx=128), dict(ldy=64), dict(xadd=v, ldxa=8), dict(r=v, ldr=64), dict(W=k + 8), dict(y=out + 1), dict(y=out + 2, dt=0)):
        assert tl(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_token_linear: ")

    def up(x=q, W=k, b=tab, hy=v, o=out, P=1, g=3, gelu_in=1):
        return lib.vdr_op_mask_upscale(x, W, b, hy, o, P, g, gelu_in, None)
    for kw in (dict(g=0), dict(g=65)):
        assert up(**kw) == -7, kw
    for kw in (dict(x=None), dict(W=None), dict(b=None), dict(hy=None), dict(o=None), dict(P=0), dict(gelu_in=2), dict(x=q + 8), dict(o=out + 4),
               dict(P=2 ** 20, g=64)):
        assert up(**kw) == -1, kw
    # well-formed calls get as far as the device check: without a device that is VDR_ERR_NO_DEVICE, after every refusal above
    if not torch.cuda.is_available():
        assert xa() == -2 and xa(tq=100, tk=7, qa=tab, ka=None) == -2 and tl() == -2 and tl(groups=4, M=8) == -2 and up() == -2


def test_mask_decoder_object_refuses_bad_arguments_before_touching_a_device():
    """every refusal of the vdr_mask_decoder_* entry points comes before the device check: without a device a well-formed
    create is VDR_ERR_NO_DEVICE, after all of them"""
    from vdr import _lib
    lib = _lib.load()
    h = C.c_void_p()

    def cfg(**kw):
        f = dict(grid=8, img=128, channels=256, heads=8, depth=2, mlp_dim=128, attention_downsample_rate=2, mask_tokens=4,
                 upscale_channels_1=64, upscale_channels_2=32, iou_head_depth=3, ln_eps=1e-5, final_ln_eps=1e-5, ln2d_eps=1e-6)
        f.update(kw)
        return _lib.vdr_mask_decoder_config(**f)

    def create(**kw):
        c = cfg(**kw)
        return lib.vdr_mask_decoder_create(C.byref(c), 0, C.byref(h))
    for kw in (dict(grid=0), dict(grid=65), dict(channels=128), dict(heads=4), dict(depth=3), dict(mlp_dim=100), dict(mlp_dim=4096), dict(mlp_dim=0),
               dict(attention_downsample_rate=1), dict(mask_tokens=3), dict(upscale_channels_1=32), dict(upscale_channels_2=16), dict(iou_head_depth=2)):
        assert create(**kw) == -7, kw     # VDR_ERR_UNSUPPORTED
        assert lib.vdr_last_error(None).startswith(b"vdr_mask_decoder_create: ") and not h.value
    for kw in (dict(img=0), dict(ln_eps=0.0), dict(final_ln_eps=-1.0), dict(ln2d_eps=float("nan"))):
        assert create(**kw) == -1, kw     # VDR_ERR_INVALID
    c = cfg()
    assert lib.vdr_mask_decoder_create(None, 0, C.byref(h)) == -1 and lib.vdr_mask_decoder_create(C.byref(c), 0, None) == -1
    assert lib.vdr_mask_decoder_create(C.byref(c), -1, C.byref(h)) == -1
    buf = (C.c_char * 256)()
    shape = (C.c_int64 * 1)(4)
    n = C.c_size_t()
    assert lib.vdr_mask_decoder_set_weight(None, b"x", buf, shape, 1) == -1
    assert lib.vdr_mask_decoder_finalize(None) == -1
    assert lib.vdr_mask_decoder_workspace_bytes(None, 1, C.byref(n)) == -1
    assert lib.vdr_mask_decode(None, buf, 0, buf, 1, 1, buf, 256, buf, buf, None) == -1
    assert lib.vdr_mask_decoder_num_weights(None) == 0 and lib.vdr_mask_decoder_weight_name(None, 0) is None
    lib.vdr_mask_decoder_destroy(None)
    if not torch.cuda.is_available():
        assert create() == -2 and b"no CPU path" in lib.vdr_last_error(None)   # VDR_ERR_NO_DEVICE, after every refusal above


def test_a_transformers_spelled_encoder_translates_back_to_the_canonical_names():
    from oracle import sam_oracle as so
    from vdr.weights import from_sam_hf_vision_state_dict
    w = so.make_weights(so.SamCfg(128, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6), seed=3, scale=0.05)
    hf = R.encoder_to_hf(w)
    assert "vision_encoder.layers.1.layer_norm2.weight" in hf and "vision_encoder.neck.conv2.weight" in hf
    assert "vision_encoder.patch_embed.projection.bias" in hf and "vision_encoder.layers.0.mlp.lin1.weight" in hf
    back = from_sam_hf_vision_state_dict({**hf, "mask_decoder.iou_token.weight": torch.zeros(1)})
    assert sorted(back) == sorted(list(w) + ["mask_decoder.iou_token.weight"]) and all(torch.equal(back[k], w[k]) for k in w)
