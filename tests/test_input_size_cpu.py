"""CPU: the input-size feature (vdr_set_input_size / vdr_get_input_size / vdr_op_interpolate_pos) at the boundary --
declarations, bindings and exports, refusals that happen before a device is touched, the host-side refusals, and the
definition the device table is tested against: the UNCHANGED oracle fed the float64-resampled position table
reproduces transformers' Dinov2Model / ViTModel(interpolate_pos_encoding=True) at other input sizes
(tests/golden/make_golden_resize.py) to the tolerance of the existing cross-check (tests/test_oracle.py: 5e-5)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_declarations_bindings_and_exports():
    from vdr import _lib
    hdr = _header()
    for decl in ("int vdr_op_interpolate_pos(const float* pos, int gh0, int gw0, int D, float* out, int gh, int gw, void* stream);",
                 "int vdr_set_input_size(vdr_handle h, int height, int width);",
                 "int vdr_get_input_size(vdr_handle h, int* height, int* width);"):
        assert decl in hdr, decl
    _P, _I = C.c_void_p, C.c_int
    assert _lib.SYMBOLS["vdr_op_interpolate_pos"] == (_I, [_P, _I, _I, _I, _P, _I, _I, _P])
    assert _lib.SYMBOLS["vdr_set_input_size"] == (_I, [_P, _I, _I])
    assert _lib.SYMBOLS["vdr_get_input_size"] == (_I, [_P, C.POINTER(_I), C.POINTER(_I)])
    lib = _lib.load()
    for name in ("vdr_op_interpolate_pos", "vdr_set_input_size", "vdr_get_input_size"):
        assert hasattr(lib, name), name
    # additive: no ABI bump, vdr_config keeps its layout
    assert lib.vdr_abi_version() == 8
    assert "#define VDR_ABI_VERSION 8" in hdr
    assert C.sizeof(_lib.vdr_config) == 100


def test_interpolate_pos_refuses_bad_arguments_before_a_device():
    from vdr import _lib
    lib = _lib.load()
    b = (C.c_char * 64)()
    ok = dict(pos=b, gh0=2, gw0=2, D=4, out=b, gh=3, gw=3)

    def call(**kw):
        a = {**ok, **kw}
        return lib.vdr_op_interpolate_pos(a["pos"], a["gh0"], a["gw0"], a["D"], a["out"], a["gh"], a["gw"], None)
    for name in ("pos", "out"):
        assert call(**{name: None}) == -1, name  # VDR_ERR_INVALID
        assert name.encode() in lib.vdr_last_error(None) and b"null" in lib.vdr_last_error(None)
    for name in ("gh0", "gw0", "D", "gh", "gw"):
        for bad in (0, -3):
            assert call(**{name: bad}) == -1, (name, bad)
            assert re.search(rb"\b" + name.encode() + rb"\b", lib.vdr_last_error(None)), (name, lib.vdr_last_error(None))


def test_set_and_get_input_size_refuse_bad_arguments_before_a_handle_or_device():
    from vdr import _lib
    lib = _lib.load()
    assert lib.vdr_set_input_size(None, 0, 16) == -1
    assert b"height" in lib.vdr_last_error(None)
    assert lib.vdr_set_input_size(None, 16, -1) == -1
    assert b"width" in lib.vdr_last_error(None)
    assert lib.vdr_set_input_size(None, 16, 16) == -1
    assert b"null" in lib.vdr_last_error(None)
    hh, ww = C.c_int(7), C.c_int(7)
    assert lib.vdr_get_input_size(None, C.byref(hh), C.byref(ww)) == -1
    assert lib.vdr_get_input_size(None, None, None) == -1
    assert (hh.value, ww.value) == (7, 7)


def test_host_refusals_without_an_engine():
    import vdr
    from vdr.engine import Engine
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.set_input_size(512, 512)
    with pytest.raises(ValueError, match="SAM"):
        VitDescriptorModel(vdr.ARCHS["medsam"], {}, dynamic_size=True)
    e = Engine.__new__(Engine)
    e.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        e.set_input_size(512, 512)
    e.cfg = vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False, has_pos=False)
    with pytest.raises(ValueError, match="token model"):
        e.set_input_size(64, 64)
    e.cfg = vdr.ARCHS["vit_base16_224"]
    for bad in ((0, 224), (224, -16), (230, 224), (224, 100)):
        with pytest.raises(ValueError, match="multiples of patch"):
            e.set_input_size(*bad)
    # an engine that was never told a size: the native geometry, and the ValueError other shapes get today
    assert e.input_size == (224, 224) and e.grid == (14, 14) and e.n_patches == 196 and e.n_tokens == 197
    with pytest.raises(ValueError, match=r"images must be \[B,3,224,224\]"):
        e.forward(torch.zeros(1, 3, 448, 448))
    e._size = (448, 224)
    assert e.grid == (28, 14) and e.n_tokens == 393


def test_native_dinov2_small_arch():
    import vdr
    from vdr.weights import expected_weight_shapes
    c = vdr.ARCHS["dinov2_small14_518"]
    assert (c.img, c.patch, c.dim, c.heads, c.layers, c.mlp_hidden, c.layerscale) == (518, 14, 384, 6, 12, 1536, True)
    assert tuple(expected_weight_shapes(c)["pos_embed"]) == (1, 1370, 384)  # a real dinov2_vits14 table loads as it is


def test_interpolate_pos_embed_host_definition():
    """The float64 definition: exact for integer tables at dyadic ratios (every cubic weight is a dyadic rational there),
    where torch's own fp32 path gives the same bits; the CLS row is copied; the native grid returns the table."""
    from vdr.weights import interpolate_pos_embed
    g = torch.Generator().manual_seed(0)
    for (g0h, g0w), (gh, gw) in (((4, 4), (8, 8)), ((8, 8), (4, 4)), ((4, 6), (16, 12))):
        t = torch.randint(-8, 9, (1, 1 + g0h * g0w, 16), generator=g).float()
        got = interpolate_pos_embed(t, (gh, gw), 1, (g0h, g0w))
        assert got.shape == (1, 1 + gh * gw, 16) and got.dtype == torch.float32
        assert torch.equal(got[0, 0], t[0, 0])
        f32 = torch.nn.functional.interpolate(t[0, 1:].reshape(1, g0h, g0w, 16).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic",
                                              align_corners=False).permute(0, 2, 3, 1).reshape(gh * gw, 16)
        assert torch.equal(got[0, 1:], f32)
    t = torch.randn(1, 17, 8, generator=g)
    assert torch.equal(interpolate_pos_embed(t, (4, 4)), t)
    with pytest.raises(ValueError):
        interpolate_pos_embed(torch.zeros(1, 16, 8), (4, 4))  # 15 patch rows are no square grid


@pytest.mark.parametrize("name", ["dinov2_hf_resize", "vit_hf_resize"])
def test_oracle_with_float64_interpolated_table_matches_transformers(golden_dir, name):
    from vdr.weights import interpolate_pos_embed
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    sw = name.startswith("dinov2")
    img, patch = int(g["img"]), int(g["patch"])
    cfg = vo.VitCfg(img, patch, 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]),
                    act="swiglu" if sw else "gelu", layerscale=sw, ln_eps=1e-6)
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    sizes = [tuple(int(v) for v in s) for s in g["sizes"]]
    assert (img, img) in sizes and any(h == w_ and h > img for h, w_ in sizes) and any(h == w_ and h < img for h, w_ in sizes)
    assert any(h > w_ for h, w_ in sizes) and any(h < w_ for h, w_ in sizes)
    for k, (H, W) in enumerate(sizes):
        x = torch.rand((int(g["batch"]), 3, H, W), generator=torch.Generator().manual_seed(int(g["xseed"]) + k), dtype=torch.float32)
        ws = dict(w)
        ws["pos_embed"] = interpolate_pos_embed(w["pos_embed"], (H // patch, W // patch))
        if (H, W) == (img, img):
            assert torch.equal(ws["pos_embed"], w["pos_embed"])  # the native entry runs on the loaded table
        o = vo.forward_images(cfg, ws, x)
        want = g[f"tokens_{H}x{W}"]
        assert o["tokens"].shape == want.shape == (int(g["batch"]), 1 + (H // patch) * (W // patch), cfg.dim)
        err = np.abs(o["tokens"].numpy() - want).max()
        print(f"{name} {H}x{W}: max|oracle - transformers| = {err:.3e}")
        assert err <= 5e-5, (H, W, err)
