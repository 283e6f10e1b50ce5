"""CPU: DINOv3 and DINOv2-with-registers -- the fp32 restatement (tests/dinov3_ref.py) against the committed transformers
vectors, the state_dict translators, the new symbols and config fields, and the refusals of vdr_create_ext and the RoPE
operators before a device is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dinov3_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = {"dinov3_hf_tiny": "dinov3", "dinov3_hf_gated_hd64": "dinov3", "dinov2reg_hf_tiny": "dinov2reg"}


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def _translated(g, family):
    from vdr import weights as W
    f = W.from_dinov3_vit_state_dict if family == "dinov3" else W.from_dinov2_hf_state_dict
    return f(dr.golden_state_dict(g))


# ---- restatement vs transformers (SURVEY 8d's fp32 gate: 2e-5 max-abs) -------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_restatement_matches_the_transformers_vectors(golden_dir, name):
    g, family = _golden(golden_dir, name), GOLDENS[name]
    rc, w = dr.golden_cfg(g, family), _translated(g, family)
    tags = [""] + (["_64x32"] if "x_64x32" in g.files else [])
    assert name != "dinov3_hf_tiny" or tags == ["", "_64x32"]
    for tag in tags:
        got = dr.forward(rc, w, torch.from_numpy(g["x" + tag]))
        for key, val in (("last_hidden_state", got["tokens"]), ("pooler_output", got["cls"])):
            want = torch.from_numpy(g[key + tag])
            err = (val - want).abs().max().item()
            print(f"{name} {key}{tag}: max |restatement - transformers| = {err:.3e} (output magnitude {want.abs().max().item():.2f})")
            assert val.shape == want.shape and err <= 2e-5, (key, tag, err)
        n = (g["x" + tag].shape[-2] // rc.vit.patch) * (g["x" + tag].shape[-1] // rc.vit.patch)
        assert got["tokens"].shape[1] == 1 + rc.n_register + n and got["dense"].shape[1] == n


def test_rope_table_statement_matches_the_definition():
    """vdr.weights.rope2d_table against the definition written out per element in Python floats (float64)."""
    from vdr.weights import rope2d_table
    for (gh, gw), dh, theta in (((3, 5), 32, 100.0), ((2, 7), 64, 100.0), ((4, 4), 128, 10000.0)):
        cos, sin = rope2d_table((gh, gw), dh, theta)
        assert cos.shape == sin.shape == (gh * gw, dh // 2) and cos.dtype == torch.float32
        for y in range(gh):
            for x in range(gw):
                for j in range(dh // 2):
                    i, coord = (j, 2 * (y + 0.5) / gh - 1) if j < dh // 4 else (j - dh // 4, 2 * (x + 0.5) / gw - 1)
                    a = 2 * math.pi * coord * theta ** (-4 * i / dh)
                    assert abs(cos[y * gw + x, j].item() - math.cos(a)) <= 2.0 ** -23 and abs(sin[y * gw + x, j].item() - math.sin(a)) <= 2.0 ** -23


# ---- translators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_translators_give_the_canonical_names_and_shapes(golden_dir, name):
    from vdr import weights as W
    g, family = _golden(golden_dir, name), GOLDENS[name]
    sd, w, rc = dr.golden_state_dict(g), _translated(g, family), dr.golden_cfg(g, family)
    cfg = dr.vdr_config(rc)
    assert {k: tuple(v.shape) for k, v in w.items()} == W.expected_weight_shapes(cfg)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in w.values())
    D, R = rc.vit.dim, rc.n_register
    assert w["register_tokens"].shape == (1, R, D) and torch.equal(w["register_tokens"], sd["embeddings.register_tokens"])
    assert not any("mask_token" in k for k in w)
    assert cfg.n_tokens == 1 + R + cfg.n_patches and cfg.n_prefix == 1 + R
    if family == "dinov3":
        assert "pos_embed" not in w
        for i in range(rc.vit.layers):
            s = f"model.layer.{i}."
            fw, fb = w[f"blocks.{i}.attn.qkv.weight"], w[f"blocks.{i}.attn.qkv.bias"]
            for j, p in enumerate("qkv"):
                assert torch.equal(fw[j * D:(j + 1) * D], sd[s + f"attention.{p}_proj.weight"])
            assert torch.equal(fb[:D], sd[s + "attention.q_proj.bias"]) and torch.equal(fb[2 * D:], sd[s + "attention.v_proj.bias"])
            assert s + "attention.k_proj.bias" not in sd and torch.count_nonzero(fb[D:2 * D]) == 0  # the zero k bias
            assert torch.equal(w[f"blocks.{i}.ls1.gamma"], sd[s + "layer_scale1.lambda1"])
            if rc.vit.act == "swiglu":
                F = rc.vit.mlp_hidden
                assert torch.equal(w[f"blocks.{i}.mlp.w12.weight"][:F], sd[s + "mlp.gate_proj.weight"])
                assert torch.equal(w[f"blocks.{i}.mlp.w12.weight"][F:], sd[s + "mlp.up_proj.weight"])
                assert torch.equal(w[f"blocks.{i}.mlp.w3.bias"], sd[s + "mlp.down_proj.bias"])
            else:
                assert torch.equal(w[f"blocks.{i}.mlp.fc1.weight"], sd[s + "mlp.up_proj.weight"])
                assert torch.equal(w[f"blocks.{i}.mlp.fc2.weight"], sd[s + "mlp.down_proj.weight"])
        # the layers without the leading `model.`
        bare = {(k[len("model."):] if k.startswith("model.layer.") else k): v for k, v in sd.items()}
        w2 = W.from_dinov3_vit_state_dict(bare)
        assert sorted(w2) == sorted(w) and all(torch.equal(w2[k], w[k]) for k in w)
        with pytest.raises(KeyError):
            W.from_dinov3_vit_state_dict({"cls_token": torch.zeros(1)})
    else:
        assert torch.equal(w["pos_embed"], sd["embeddings.position_embeddings"]) and w["pos_embed"].shape == (1, 1 + cfg.n_patches, D)
        assert torch.equal(w["blocks.1.attn.qkv.bias"][D:2 * D], sd["encoder.layer.1.attention.attention.key.bias"])
        assert torch.equal(w["norm.bias"], sd["layernorm.bias"])
        # a plain transformers Dinov2Model state_dict (no registers) translates to the DINOv2 the library already runs
        w2 = W.from_dinov2_hf_state_dict({k: v for k, v in sd.items() if k != "embeddings.register_tokens"})
        import vdr
        plain = vdr.VdrConfig(**{**cfg.__dict__, "n_register": 0})
        assert {k: tuple(v.shape) for k, v in w2.items()} == W.expected_weight_shapes(plain)
        with pytest.raises(KeyError):
            W.from_dinov2_hf_state_dict({"cls_token": torch.zeros(1)})


def test_architectures_of_the_two_families():
    import vdr
    for name, (D, H, Lr, F, act) in {"dinov3_vits16": (384, 6, 12, 1536, "gelu"), "dinov3_vits16plus": (384, 6, 12, 1536, "swiglu"),
                                     "dinov3_vitb16": (768, 12, 12, 3072, "gelu"), "dinov3_vitl16": (1024, 16, 24, 4096, "gelu"),
                                     "dinov3_vith16plus": (1280, 20, 32, 5120, "swiglu")}.items():
        a = vdr.ARCHS[name]
        assert (a.dim, a.heads, a.layers, a.mlp_hidden, a.act) == (D, H, Lr, F, act), name
        assert (a.img, a.patch, a.n_register, a.rope, a.has_pos, a.layerscale, a.has_cls, a.pre_ln) == (224, 16, 4, True, False, True, True, True)
        assert a.ln_eps == pytest.approx(1e-5) and a.rope_theta == 100.0 and a.n_tokens == 1 + 4 + 196
    for name, (D, H, Lr, F, act) in {"dinov2_small14_reg_518": (384, 6, 12, 1536, "gelu"), "dinov2_base14_reg_518": (768, 12, 12, 3072, "gelu"),
                                     "dinov2_large14_reg_518": (1024, 16, 24, 4096, "gelu"),
                                     "dinov2_giant14_reg_518": (1536, 24, 40, 4096, "swiglu")}.items():
        a = vdr.ARCHS[name]
        assert (a.dim, a.heads, a.layers, a.mlp_hidden, a.act) == (D, H, Lr, F, act), name
        assert (a.img, a.patch, a.n_register, a.rope, a.has_pos, a.layerscale) == (518, 14, 4, False, True, True)
        assert a.ln_eps == pytest.approx(1e-6) and a.n_tokens == 1 + 4 + 37 * 37


def test_header_and_bindings_declare_the_new_symbols():
    import vdr
    from vdr import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdr.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in ("vdr_create_ext", "vdr_op_rope2d", "vdr_op_rope2d_table"):
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define VDR_ABI_VERSION 8\b", hdr) and lib.vdr_abi_version() == 8
    assert C.sizeof(_lib.vdr_config) == 100  # frozen: the new geometry travels in vdr_config_ext
    m = re.search(r"typedef struct \{([^}]*)\} vdr_config_ext;", hdr)
    assert m and re.findall(r"(int32_t|float)\s+(\w+);", m.group(1)) == [("int32_t", "size"), ("int32_t", "n_register"),
                                                                          ("int32_t", "rope"), ("float", "rope_theta")]
    assert [f[0] for f in _lib.vdr_config_ext._fields_] == ["size", "n_register", "rope", "rope_theta"] and C.sizeof(_lib.vdr_config_ext) == 16
    cfg = vdr.VdrConfig(n_register=4, rope=True, rope_theta=50.0, has_pos=False)
    e = cfg.to_c_ext()
    assert (e.size, e.n_register, e.rope, e.rope_theta) == (16, 4, 1, 50.0)
    d = vdr.VdrConfig().to_c_ext()
    assert (d.size, d.n_register, d.rope, d.rope_theta) == (16, 0, 0, 100.0)
    assert C.sizeof(cfg.to_c()) == 100 and vdr.VdrConfig().n_tokens == 197 and cfg.n_tokens == 201
    assert callable(ops.rope2d) and callable(ops.rope2d_table)


# ---- refusals before a device is touched ---------------------------------------------------------------------------------
UNSUPPORTED, INVALID, NO_DEVICE = -7, -1, -2


def _create_ext(ext=None, raw_ext=None, **kw):
    import vdr
    from vdr import _lib
    lib = _lib.load()
    cfg = vdr.VdrConfig(**kw)
    cc = cfg.to_c()
    h = C.c_void_p()
    if raw_ext is None and ext is not None:
        raw_ext = _lib.vdr_config_ext(16, ext.get("n_register", 0), ext.get("rope", 0), ext.get("rope_theta", 100.0))
    rc = lib.vdr_create_ext(C.byref(cc), C.byref(raw_ext) if raw_ext is not None else None, 0, C.byref(h))
    msg = lib.vdr_last_error(None)
    if rc == 0:
        lib.vdr_destroy(h)
    return rc, msg


DINOV3 = dict(has_pos=False, layerscale=True, ln_eps=1e-5)


def test_create_ext_refusals_before_touching_a_device():
    for ext, what in (({"n_register": 4}, b"n_register > 0"), ({"rope": 1}, b"rope = 1")):
        base = DINOV3 if ext.get("rope") else {}
        rc, msg = _create_ext(ext, fp8=1, **base)
        assert rc == UNSUPPORTED and what in msg and b"fp8" in msg, (ext, rc, msg)
        rc, msg = _create_ext(ext, img=0, patch=0, in_chans=0, has_pos=False, input_ln=True)
        assert rc == UNSUPPORTED and what in msg and b"patch == 0" in msg, (ext, rc, msg)
        rc, msg = _create_ext(ext, pre_ln=False, **base)
        assert rc == UNSUPPORTED and what in msg and b"pre-LN" in msg, (ext, rc, msg)
    rc, msg = _create_ext({"rope": 1}, img=1024, has_cls=False, window=14, global_blocks=(2, 5, 8, 11), neck_chans=256)
    assert rc == UNSUPPORTED and b"window > 0" in msg, (rc, msg)
    rc, msg = _create_ext({"rope": 1}, has_pos=True)
    assert rc == UNSUPPORTED and b"has_pos = 1" in msg, (rc, msg)
    rc, msg = _create_ext({"rope": 1}, dim=192, heads=2, mlp_hidden=768, **DINOV3)  # head dim 96
    assert rc == UNSUPPORTED and b"head dim" in msg and b"96" in msg, (rc, msg)
    rc, msg = _create_ext({"n_register": 17})
    assert rc == UNSUPPORTED and b"at most 16" in msg, (rc, msg)
    rc, msg = _create_ext({"n_register": 4}, has_cls=False)
    assert rc == INVALID and b"has_cls" in msg, (rc, msg)
    rc, msg = _create_ext({"n_register": -1})
    assert rc == INVALID and b"n_register" in msg, (rc, msg)
    for theta in (float("nan"), float("inf"), 1.0, 0.5, -100.0):
        rc, msg = _create_ext({"rope": 1, "rope_theta": theta}, **DINOV3)
        assert rc == INVALID and b"rope_theta" in msg, (theta, rc, msg)
    from vdr import _lib
    for size in (0, 8, 12, 15, -16):
        rc, msg = _create_ext(raw_ext=_lib.vdr_config_ext(size, 4, 0, 100.0))
        assert rc == INVALID and b"size" in msg, (size, rc, msg)


def test_accepted_configs_and_plain_create_reach_the_device_check():
    """What is not refused goes on to the device (VDR_OK with one, VDR_ERR_NO_DEVICE without); vdr_create and a null ext are
    exactly what they were."""
    import vdr
    from vdr import _lib
    lib = _lib.load()
    want = (0,) if lib.vdr_device_count() > 0 else (NO_DEVICE,)
    assert _create_ext(None)[0] in want                                            # ext = NULL
    assert _create_ext({"n_register": 4})[0] in want and _create_ext({"n_register": 16})[0] in want
    assert _create_ext({"n_register": 4, "rope": 1}, **DINOV3)[0] in want
    assert _create_ext({"rope": 1, "rope_theta": 10000.0}, dim=256, heads=2, mlp_hidden=512, **DINOV3)[0] in want  # head dim 128
    assert _create_ext({"n_register": 0, "rope": 0, "rope_theta": float("nan")})[0] in want  # (theta is read with rope = 1 only)
    bigger = (C.c_int32 * 8)(32, 4, 0, 0, 0, 0, 0, 0)  # a later caller's larger struct: the known fields are read
    bigger[3] = C.c_int32.from_buffer_copy(C.c_float(100.0)).value
    assert _create_ext(raw_ext=C.cast(bigger, C.POINTER(_lib.vdr_config_ext)).contents)[0] in want
    h = C.c_void_p()
    for kw, code, text in ((dict(), want[0], None), (dict(dim=100), UNSUPPORTED, b"head dim"), (dict(img=225), INVALID, b"multiple of patch"),
                           (dict(fp8=1, pre_ln=False, has_pos=False), UNSUPPORTED, b"pre-LN")):
        cc = vdr.VdrConfig(**kw).to_c()
        rc = lib.vdr_create(C.byref(cc), 0, C.byref(h))
        assert rc == code and (text is None or text in lib.vdr_last_error(None)), (kw, rc, lib.vdr_last_error(None))
        if rc == 0:
            lib.vdr_destroy(h)


def test_rope_ops_refuse_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    al = (base + 15) // 16 * 16
    for dh in (0, 16, 48, 96, 256):
        assert lib.vdr_op_rope2d_table(3, 5, dh, 100.0, al, al, None) == UNSUPPORTED and b"head_dim" in lib.vdr_last_error(None)
        assert lib.vdr_op_rope2d(al, 1, 4, 1, 1, dh, al, al, None) == UNSUPPORTED and b"head_dim" in lib.vdr_last_error(None)
    assert lib.vdr_op_rope2d_table(3, 5, 32, 100.0, None, al, None) == INVALID
    assert lib.vdr_op_rope2d_table(0, 5, 32, 100.0, al, al, None) == INVALID
    assert lib.vdr_op_rope2d_table(3, 5, 32, 1.0, al, al, None) == INVALID and b"theta" in lib.vdr_last_error(None)
    assert lib.vdr_op_rope2d(None, 1, 4, 1, 1, 32, al, al, None) == INVALID
    assert lib.vdr_op_rope2d(al, 1, 4, 5, 1, 32, al, al, None) == INVALID   # prefix > seq
    assert lib.vdr_op_rope2d(al, 0, 4, 1, 1, 32, al, al, None) == INVALID
    assert lib.vdr_op_rope2d(al + 2, 1, 4, 1, 1, 32, al, al, None) == INVALID and b"aligned" in lib.vdr_last_error(None)
