"""CPU: head dims 32, 96 and 128 (dim / heads) next to 64 -- the configurations vdr_create takes and refuses, the
vdr_op_attention_hd entry point, the ISA of csrc/attention_hd.hip, and the oracle against the golden vectors the
reference's own classifiers produced at those head dims (tests/golden/make_golden_headdim.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(**kw):
    import vdr
    from vdr import _lib
    lib = _lib.load()
    h = C.c_void_p()
    cc = vdr.VdrConfig(**kw).to_c()
    rc = lib.vdr_create(C.byref(cc), 0, C.byref(h))
    if rc == 0:
        lib.vdr_destroy(h)
    return rc, (lib.vdr_last_error(None) or b"")


TOKEN_MODEL = dict(img=0, patch=0, in_chans=0, act="gelu", pre_ln=False, layerscale=False, has_cls=True, has_pos=False,
                   input_ln=True, ln_eps=1e-5, layers=2)


@pytest.mark.parametrize("dim,heads", [(384, 4), (256, 8), (256, 2)])
def test_supported_head_dims_are_accepted(dim, heads):
    rc, msg = _create(dim=dim, heads=heads, mlp_hidden=4 * dim, **TOKEN_MODEL)
    assert rc == (0 if torch.cuda.is_available() else -2), (rc, msg)  # -2: VDR_ERR_NO_DEVICE (checked after the config)
    # a bf16 pre-LN image model without windows too
    rc, msg = _create(img=64, patch=16, dim=dim, heads=heads, layers=2, mlp_hidden=2 * dim)
    assert rc == (0 if torch.cuda.is_available() else -2), (rc, msg)


def test_unsupported_head_dims_are_refused():
    for kw in (dict(dim=100, heads=2, mlp_hidden=256, **TOKEN_MODEL),   # dh 50
               dict(dim=256, heads=1, mlp_hidden=1024, **TOKEN_MODEL),  # dh 256
               dict(img=64, patch=16, dim=384, heads=4, layers=2, mlp_hidden=1536, fp8=1)):  # MX-fp8: dh 64 only
        rc, msg = _create(**kw)
        assert rc == -7 and b"head dim" in msg, (kw, rc, msg)
    # SAM-shaped (windowed attention, rel-pos tables [2S-1, 64]): dh 96 refused, the same model at dh 64 is not
    sam = dict(img=224, patch=16, layers=2, window=14, has_cls=False, has_pos=True, neck_chans=256)
    rc, msg = _create(dim=384, heads=4, mlp_hidden=1536, **sam)
    assert rc == -7 and b"head dim" in msg, (rc, msg)
    rc, msg = _create(dim=384, heads=6, mlp_hidden=1536, **sam)
    assert rc == (0 if torch.cuda.is_available() else -2), (rc, msg)


def test_attention_hd_is_declared_bound_and_exported():
    from vdr import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdr.h")).read(), flags=re.S)
    assert re.search(r"int vdr_op_attention_hd\(const void\* qkv, void\* out, int batch, int seq, int heads, int head_dim,\s*"
                     r"int variant,\s*void\* stream\);", hdr)
    assert "vdr_op_attention_hd" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_attention_hd")
    assert lib.vdr_abi_version() == 8
    buf = (C.c_char * 64)()
    for bad in (0, 16, 48, 80, 256):  # refused before any device is looked for
        assert lib.vdr_op_attention_hd(buf, buf, 1, 1, 1, bad, 0, None) == -7
        assert b"head dim" in lib.vdr_last_error(None)
    if not torch.cuda.is_available():
        assert lib.vdr_op_attention_hd(buf, buf, 1, 1, 1, 96, 0, None) == -2


def test_attention_hd_kernels_compile_without_scratch():
    """One kernel per head dim (32, 96, 128), every one without spills (ScratchSize 0), and LDS small enough for at least
    two workgroups per CU (160 KiB)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("hazard_scan", os.path.join(ROOT, "tools", "hazard_scan.py"))
    hs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hs)
    (isa,) = hs.compile_isa([os.path.join(hs.CSRC, "attention_hd.hip")], jobs=1)
    txt = open(isa).read()
    kernels = re.findall(r"^(_ZN3vdr\S*attn_hd_kernelILi(\d+)\S*):\s*; @\S+\n.*?; ScratchSize: (\d+)", txt, re.S | re.M)
    assert sorted(int(k[1]) for k in kernels) == [32, 96, 128], [k[0] for k in kernels]
    for name, _, scratch in kernels:
        assert int(scratch) == 0, (name, scratch)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", txt)]
    assert len(lds) == 3 and all(0 < v <= 80 * 1024 for v in lds), lds


@pytest.mark.parametrize("tag", ["hd96", "hd32", "hd128"])
def test_postln_oracle_matches_reference_at_head_dim(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, f"postln_{tag}.npz"), allow_pickle=False)
    dim, heads = int(g["dim"]), int(g["heads"])
    assert dim // heads == {"hd96": 96, "hd32": 32, "hd128": 128}[tag]
    cfg = vo.postln_cfg(dim, heads, int(g["layers"]), int(g["ffn"]))
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = vo.make_tokens(int(g["batch"]), int(g["seq"]), dim, seed=int(g["xseed"]))
    np.testing.assert_array_equal(x[0, :2, :8].numpy(), g["x_probe"])
    np.testing.assert_array_equal(w["blocks.0.attn.qkv.weight"][:2, :8].numpy(), g["w_probe"])
    o = vo.forward_tokens(cfg, w, x)
    assert np.abs(o["cls"].numpy() - g["cls"]).max() <= 2e-5
    logits = vo.mlp_head(o["cls"], *(torch.from_numpy(g["head.classifier." + k])
                                     for k in ("dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias")))
    assert np.abs(logits.numpy() - g["logits"]).max() <= 2e-5


def test_bimodal_oracle_matches_reference_at_head_dims(golden_dir):
    from oracle import bimodal_oracle as bo
    g = np.load(os.path.join(golden_dir, "bimodal_hd.npz"), allow_pickle=False)
    dim, lc, lp = int(g["dim"]), int(g["layers_ct"]), int(g["layers_pet"])
    assert (dim // int(g["heads_ct"]), dim // int(g["heads_pet"])) == (96, 128)
    fc, fp = int(float(g["ratio_ct"]) * dim), int(float(g["ratio_pet"]) * dim)
    sd = bo.make_state_dict(dim, fc, fp, lc, lp, int(g["classes"]), seed=int(g["seed"]))
    assert np.array_equal(sd["cross_attention_ct.multihead_attn.in_proj_weight"][:2, :8].numpy(), g["w_probe"])
    x_ct, x_pet = torch.from_numpy(g["x_ct"]), torch.from_numpy(g["x_pet"])
    for mode, (a, b) in (("both", (x_ct, x_pet)), ("ct", (x_ct, None)), ("pet", (None, x_pet))):
        out = bo.forward(sd, dim, fc, fp, int(g["heads_ct"]), int(g["heads_pet"]), lc, lp, a, b)
        for name, o in zip(("logits_petct", "cls_petct", "logits_ct", "logits_pet"), out):
            want = torch.from_numpy(g[f"{mode}_{name}"])
            assert o.shape == want.shape and (o - want).abs().max().item() < 2e-5, (mode, name)
