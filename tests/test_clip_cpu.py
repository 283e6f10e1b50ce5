"""CPU: CLIP / SigLIP vision towers -- the fp32 restatement (tests/clip_ref.py) against the committed transformers
vectors, the state_dict translators, the device activation formulas evaluated in fp32, and the refusals of the new
config values and of vdr_op_attention_pool before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir, family):
    return np.load(os.path.join(golden_dir, family + "_hf_tiny.npz"), allow_pickle=False)


def _translated(g, family):
    from vdr import weights as W
    f = W.from_clip_vision_state_dict if family == "clip" else W.from_siglip_vision_state_dict
    return f(cr.golden_state_dict(g))


# ---- restatement vs transformers (SURVEY 8d's fp32 gate: 2e-5 max-abs) -------------------------------------------------
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_restatement_matches_the_transformers_vectors(golden_dir, family):
    g = _golden(golden_dir, family)
    cfg, w = cr.tiny_cfg(g, family), _translated(g, family)
    fwd = cr.clip_forward if family == "clip" else cr.siglip_forward
    names = ("last_hidden_state", "pooler_output", "image_embeds") if family == "clip" else ("last_hidden_state", "pooler_output")
    got = fwd(cfg, w, torch.from_numpy(g["x"]))
    for n in names:
        err = (got[n] - torch.from_numpy(g[n])).abs().max().item()
        print(f"{family} {n}: max |restatement - transformers| = {err:.3e}")
        assert got[n].shape == g[n].shape and err <= 2e-5, (n, err)
    got = fwd(cfg, w, torch.from_numpy(g["x_64x32"]))  # interpolate_pos_encoding=True at 64 x 32
    names = ("last_hidden_state", "image_embeds") if family == "clip" else ("last_hidden_state", "pooler_output")
    for n in names:
        err = (got[n] - torch.from_numpy(g[n + "_64x32"])).abs().max().item()
        print(f"{family} {n} 64x32: max |restatement - transformers| = {err:.3e}")
        assert err <= 2e-5, (n, err)


def test_layer_norm_eps_of_the_architectures_is_what_transformers_uses(golden_dir):
    """The goldens record config.layer_norm_eps of the transformers defaults: CLIP 1e-5, SigLIP 1e-6."""
    import vdr
    assert float(_golden(golden_dir, "clip")["ln_eps"]) == pytest.approx(1e-5) and float(_golden(golden_dir, "siglip")["ln_eps"]) == pytest.approx(1e-6)
    for name in ("clip_vit_base16_224", "clip_vit_base32_224", "clip_vit_large14_336"):
        a = vdr.ARCHS[name]
        assert (a.act, a.input_ln, a.has_cls, a.pre_ln) == ("quick_gelu", True, True, True) and a.ln_eps == pytest.approx(1e-5)
    for name in ("siglip_base16_224", "siglip_large16_256"):
        a = vdr.ARCHS[name]
        assert (a.act, a.input_ln, a.has_cls, a.pre_ln) == ("gelu_tanh", False, False, True) and a.ln_eps == pytest.approx(1e-6)
    assert (vdr.ARCHS["clip_vit_base32_224"].patch, vdr.ARCHS["clip_vit_large14_336"].img, vdr.ARCHS["siglip_large16_256"].img) == (32, 336, 256)


# ---- translators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_translators_give_the_canonical_names_and_shapes(golden_dir, family):
    import vdr
    from vdr import weights as W
    g = _golden(golden_dir, family)
    sd = cr.golden_state_dict(g)
    w = _translated(g, family)
    c = cr.tiny_cfg(g, family)
    cfg = vdr.VdrConfig(c.img, c.patch, 3, c.dim, c.heads, c.layers, c.mlp_hidden, act=c.act, has_cls=c.has_cls, input_ln=c.input_ln,
                        ln_eps=c.ln_eps)
    enc, head = W.split_head_weights(w)
    assert {k: tuple(v.shape) for k, v in enc.items()} == W.expected_weight_shapes(cfg)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in w.values())
    pre = "vision_model." if family == "clip" else ""
    D = c.dim
    for i in range(c.layers):  # qkv rows: q, then k, then v
        for t in ("weight", "bias"):
            fused = w[f"blocks.{i}.attn.qkv.{t}"]
            for j, p in enumerate("qkv"):
                assert torch.equal(fused[j * D:(j + 1) * D], sd[f"{pre}encoder.layers.{i}.self_attn.{p}_proj.{t}"])
    assert torch.equal(w["pos_embed"][0], sd[pre + "embeddings.position_embedding.weight"])
    assert torch.equal(w["norm.weight"], sd[pre + "post_layernorm.weight"])
    if family == "clip":
        assert torch.equal(w["cls_token"].reshape(-1), sd["vision_model.embeddings.class_embedding"])
        assert torch.equal(w["input_norm.bias"], sd["vision_model.pre_layrnorm.bias"])
        assert torch.count_nonzero(w["patch_embed.proj.bias"]) == 0  # CLIP's conv has no bias
        assert sorted(head) == ["head.visual_projection.weight"] and head["head.visual_projection.weight"].shape == (int(g["proj"]), D)
        # CLIPVisionModel (no projection) translates too, and a prefix-free dict as well
        plain = {k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}
        w2 = W.from_clip_vision_state_dict(plain)
        assert not any(k.startswith("head.") for k in w2) and all(torch.equal(w2[k], w[k]) for k in w2)
    else:
        assert torch.equal(w["patch_embed.proj.bias"], sd["embeddings.patch_embedding.bias"])
        assert {"head.probe", "head.attention.in_proj_weight", "head.mlp.fc2.bias", "head.layernorm.weight"} <= set(head) and len(head) == 11
        w2 = W.from_siglip_vision_state_dict({"vision_model." + k: v for k, v in sd.items()})  # older transformers' prefix
        assert all(torch.equal(w2[k], w[k]) for k in w)
    with pytest.raises(KeyError):
        W.from_clip_vision_state_dict({"cls_token": torch.zeros(1)})


def test_config_and_bindings_know_the_new_values():
    import vdr
    from vdr import _lib
    from vdr import weights as W
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdr.h")).read(), flags=re.S)
    assert re.search(r"VDR_ACT_QUICK_GELU = 2,", hdr) and re.search(r"VDR_ACT_GELU_TANH = 3\b", hdr)
    assert re.search(r"VDR_EPI_BIAS_QUICK_GELU = 8,", hdr) and re.search(r"VDR_EPI_BIAS_GELU_TANH = 9\b", hdr)
    assert re.search(r"#define VDR_ABI_VERSION 8\b", hdr) and C.sizeof(_lib.vdr_config) == 100
    assert (_lib.ACT_QUICK_GELU, _lib.ACT_GELU_TANH, vdr.EPI_BIAS_QUICK_GELU, vdr.EPI_BIAS_GELU_TANH) == (2, 3, 8, 9)
    # (the internal Epilogue enum names the two activations 8 and 9 as well: a static_assert in csrc/vdr_api.hip ties them)
    for act, val in (("gelu", 0), ("swiglu", 1), ("quick_gelu", 2), ("gelu_tanh", 3)):
        assert vdr.VdrConfig(act=act).to_c().act == val
    base = W.expected_weight_shapes(vdr.VdrConfig(act="gelu"))
    assert W.expected_weight_shapes(vdr.VdrConfig(act="quick_gelu")) == base == W.expected_weight_shapes(vdr.VdrConfig(act="gelu_tanh"))
    assert "vdr_op_attention_pool" in _lib.SYMBOLS and hasattr(_lib.load(), "vdr_op_attention_pool")
    from vdr import ops
    assert callable(ops.attention_pool) and callable(vdr.VitDescriptorModel.get_image_features)


# ---- the device activation formulas in fp32 ----------------------------------------------------------------------------
def _flip_share(y32, exact64):
    """share of values whose bf16 rounding differs from the correctly rounded one (bf16 of the float64 value)"""
    good = exact64.to(torch.float32).to(torch.bfloat16)  # (fp32 keeps 16 more bits than bf16: no double-rounding case in practice)
    return (y32.to(torch.bfloat16) != good).double().mean().item()


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu_tanh"])
def test_device_activation_formula_in_fp32(kind):
    """x / (1 + 2^(e2)) with e2 = -t log2 e, every step one fp32 rounding (csrc/vdr_dev.h), against float64.
    Error bound, from the operation count: e2 carries at most 5 roundings (tanh form: x^2, the fma, the product, two
    rounded constants), 2^e2 multiplies an absolute error of e2 by ln 2, then one rounding each for exp2, the add, the
    reciprocal and the last product: relative error <= (3.5 |e2| + 4) 2^-24, checked per element wherever the result
    is a normal fp32 number."""
    x = torch.cat([torch.linspace(-12.0, 12.0, 2_000_001, dtype=torch.float64).to(torch.float32),
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38, 65504.0, -65504.0, 1e20, -1e20, 3.0e38, -3.0e38,
                                 torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max, torch.finfo(torch.float32).tiny],
                                dtype=torch.float32)])
    y = cr.device_activation_fp32(x, kind)
    ex = cr.exact_activation_fp64(x, kind)
    assert torch.isfinite(y).all(), "finite for every finite input"
    if kind == "gelu_tanh":  # the cancellation-free float64 form IS torch's gelu(approximate="tanh"), to float64's absolute resolution
        named = torch.nn.functional.gelu(x.double(), approximate="tanh")
        assert ((named - ex).abs() <= 1e-15 * x.double().abs()).all()  # (a few float64 ulp of x)
    else:
        assert torch.equal(ex, x.double() * torch.sigmoid(1.702 * x.double()))
    big = x.abs() >= 1e20
    assert torch.equal(y[big & (x > 0)], x[big & (x > 0)]) and (y[big & (x < 0)] == 0).all() and torch.signbit(y[big & (x < 0)]).all()
    t = 1.702 * x.double() if kind == "quick_gelu" else 2 * 0.7978845608028654 * (x.double() + 0.044715 * x.double() ** 3)
    e2 = (t * cr.LOG2E).abs()
    normal = ex.abs() >= 2.0 ** -100
    rel = ((y.double() - ex).abs() / ex.abs())[normal]
    bound = ((3.5 * e2 + 4) * 2.0 ** -24)[normal]
    print(f"{kind}: largest relative error {rel.max().item():.3e} (2^{np.log2(rel.max().item()):.1f}) over [-12, 12] and the extremes; "
          f"worst error / bound {(rel / bound).max().item():.3f}")
    assert (rel <= bound).all()
    assert ((y.double() - ex).abs()[~normal] <= 2.0 ** -100).all()
    sweep = _flip_share(y[:2_000_001], ex[:2_000_001])
    # the GPU gate's inputs: the share of bf16 roundings the formula ALONE flips must stay at or under a quarter of the
    # 1e-3 cap tests/test_clip_ops_gpu.py applies to the kernels
    pre = torch.cat([cr.exact_preactivation(*cr.epilogue_test_inputs(M, N, K, seed)).reshape(-1)
                     for (M, N, K, seed) in ((512, 1536, 256, 5), (333, 1000, 128, 6), (300, 1024, 768, 7))])
    assert 1.2 <= pre.std().item() <= 1.9  # (what an fc1 sees)
    share = _flip_share(cr.device_activation_fp32(pre, kind), cr.exact_activation_fp64(pre, kind))
    print(f"{kind}: bf16 roundings that differ from the correctly rounded value: {sweep:.3e} of the sweep, {share:.3e} of "
          f"{pre.numel()} GEMM-test pre-activations")
    assert share <= 2.5e-4
    # within one bf16 ulp of the correctly rounded value down to where the formula's range ends: from e2 = 126 on, 2^e2 or
    # its reciprocal leaves the normal fp32 range and the result is -0 for a true value of |x| 2^-e2 <= |x| 2^-126 (x < -10
    # in the tanh form): an absolute error of that size
    ulp_ok = (y.to(torch.bfloat16).view(torch.int16).int() - ex.to(torch.float32).to(torch.bfloat16).view(torch.int16).int()).abs() <= 1
    assert (ulp_ok | (ex.abs() <= x.double().abs() * 2.0 ** -125)).all()


# ---- refusals before a device is touched ---------------------------------------------------------------------------------
def _create(**kw):
    import vdr
    from vdr import _lib
    lib = _lib.load()
    act = kw.pop("act_value", None)
    cc = vdr.VdrConfig(**kw).to_c()
    if act is not None:
        cc.act = act
    h = C.c_void_p()
    return lib.vdr_create(C.byref(cc), 0, C.byref(h)), lib.vdr_last_error(None)


def test_create_refuses_new_activation_combinations_before_touching_a_device():
    for act in ("quick_gelu", "gelu_tanh"):
        rc, msg = _create(act=act, fp8=1)
        assert rc == -7 and b"fp8" in msg, (act, rc, msg)  # VDR_ERR_UNSUPPORTED
        rc, msg = _create(img=1024, act=act, has_cls=False, window=14, global_blocks=(2, 5, 8, 11), neck_chans=256)
        assert rc == -1 and b"SAM encoder" in msg, (act, rc, msg)
    for v in (4, 7, -1, 100):
        rc, msg = _create(act_value=v)
        assert rc == -1 and b"unknown activation" in msg, (v, rc, msg)


def test_attention_pool_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ok = [buf, buf, 128, buf, 1, 1, 1, 64, None]  # q, kv, ldkv, out, batch, n, heads, head_dim, stream

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.vdr_op_attention_pool(*a)
    for i in (0, 1, 3):
        assert call(**{f"a{i}": None}) == -1, i  # VDR_ERR_INVALID
        assert b"null" in lib.vdr_last_error(None)
    for dh in (0, 16, 48, 72, 256):
        assert call(a7=dh) == -7  # VDR_ERR_UNSUPPORTED (72: SigLIP-so400m's head dim)
        assert b"head dim" in lib.vdr_last_error(None)
    for n in (0, -3):
        assert call(a5=n) == -1 and b"n must be at least 1" in lib.vdr_last_error(None)
    assert call(a4=0) == -1 and call(a6=0) == -1
    assert call(a2=64) == -1 and call(a2=132) == -1  # ldkv < 2 D, ldkv % 8
    import vdr
    h = C.c_void_p()
    cc = vdr.VdrConfig(dim=1152, heads=16, mlp_hidden=4304 // 64 * 64, act="gelu_tanh", has_cls=False).to_c()  # so400m: head dim 72
    assert lib.vdr_create(C.byref(cc), 0, C.byref(h)) == -7 and b"head dim" in lib.vdr_last_error(None)


def test_8phase_activation_kernels_have_no_vector_memory_instruction_their_counted_waits_do_not_know():
    """The rule tests/test_abi_cpu.py states for csrc/gemm_8p.hip, for the QuickGELU / tanh-GELU instantiations of the same
    kernel (csrc/gemm_8p_act.hip): scratch size 0, and every vector-memory instruction an LDS-DMA or a buffer store."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("hazard_scan", os.path.join(ROOT, "tools", "hazard_scan.py"))
    hs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hs)
    (isa,) = hs.compile_isa([os.path.join(hs.CSRC, "gemm_8p_act.hip")], jobs=1)
    txt = open(isa).read()
    kernels = re.findall(r"^(_ZN3vdr\S*gemm_8p_kernel\S*):\s*; @\S+\n(.*?); ScratchSize: (\d+)", txt, re.S | re.M)
    assert len(kernels) == 4, [k[0] for k in kernels]
    for name, body, scratch in kernels:
        assert int(scratch) == 0, (name, scratch)
        vmem = re.findall(r"^\s+((?:global|buffer|flat|scratch)_\w+)", body, re.M)
        assert vmem and set(vmem) <= {"global_load_lds_dwordx4", "buffer_store_dwordx4"}, (name, sorted(set(vmem)))
    n, hits = hs.scan(isa, 4)
    assert not hits, hits[:3]
