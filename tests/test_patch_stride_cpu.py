"""CPU: the patch-stride feature (vdr_set_patch_stride / vdr_get_patch_stride / vdr_op_patch_embed_strided) at the boundary
-- declarations, bindings and exports, the refusals that happen before a handle or a device is touched, the host-side
refusals and grid arithmetic, and the definition the device is tested against (tests/stride_ref.py): at stride == patch it
is oracle.vit_oracle.forward_images, and its position rule is vdr.weights.interpolate_pos_embed."""
import ctypes as C
import os
import re

import pytest
import torch

import stride_ref as sr
from oracle import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_declarations_bindings_and_exports():
    from vdr import _lib
    hdr = _header()
    for decl in ("int vdr_set_patch_stride(vdr_handle h, int stride);",
                 "int vdr_get_patch_stride(vdr_handle h, int* stride);",
                 "int vdr_op_patch_embed_strided(const void* images, int in_dtype, const void* W, const float* bias, "
                 "const float* pos, void* col, void* y, int batch, int C, int H, int Wd, int p, int stride, int D, "
                 "int row_stride, int row_offset, void* stream);"):
        assert decl in hdr, decl
    _P, _I = C.c_void_p, C.c_int
    assert _lib.SYMBOLS["vdr_set_patch_stride"] == (_I, [_P, _I])
    assert _lib.SYMBOLS["vdr_get_patch_stride"] == (_I, [_P, C.POINTER(_I)])
    assert _lib.SYMBOLS["vdr_op_patch_embed_strided"] == (_I, [_P, _I, _P, _P, _P, _P, _P] + [_I] * 9 + [_P])
    lib = _lib.load()
    for name in ("vdr_set_patch_stride", "vdr_get_patch_stride", "vdr_op_patch_embed_strided"):
        assert hasattr(lib, name), name
    # additive: no ABI bump, the config structs keep their layouts, vdr_op_patch_embed its signature
    assert lib.vdr_abi_version() == 8
    assert "#define VDR_ABI_VERSION 8" in hdr
    assert C.sizeof(_lib.vdr_config) == 100
    assert C.sizeof(_lib.vdr_config_ext) == 16
    assert _lib.SYMBOLS["vdr_op_patch_embed"] == (_I, [_P, _I, _P, _P, _P, _P, _P] + [_I] * 7 + [_P])


def test_set_and_get_refuse_bad_arguments_before_a_handle_or_device():
    """the order of the header: stride <= 0, then the null handle"""
    from vdr import _lib
    lib = _lib.load()
    for bad in (0, -8):
        assert lib.vdr_set_patch_stride(None, bad) == -1  # VDR_ERR_INVALID
        assert b"stride must be positive" in lib.vdr_last_error(None)
    assert lib.vdr_set_patch_stride(None, 8) == -1
    assert b"null handle" in lib.vdr_last_error(None)
    s = C.c_int(7)
    assert lib.vdr_get_patch_stride(None, C.byref(s)) == -1 and s.value == 7
    assert lib.vdr_get_patch_stride(None, None) == -1


def test_op_refuses_bad_arguments_before_a_device():
    from vdr import _lib
    lib = _lib.load()
    b = (C.c_char * 64)()
    ok = dict(images=b, in_dtype=0, W=b, bias=None, pos=None, col=b, y=b, batch=1, C=1, H=32, Wd=32, p=16, stride=8, D=64)

    def call(**kw):
        a = {**ok, **kw}
        return lib.vdr_op_patch_embed_strided(a["images"], a["in_dtype"], a["W"], a["bias"], a["pos"], a["col"], a["y"], a["batch"],
                                              a["C"], a["H"], a["Wd"], a["p"], a["stride"], a["D"], 9, 0, None)
    for name in ("images", "W", "col", "y"):
        assert call(**{name: None}) == -1 and b"null" in lib.vdr_last_error(None), name
    assert call(in_dtype=2) == -1 and b"in_dtype" in lib.vdr_last_error(None)
    for name in ("batch", "C", "D", "p"):
        assert call(**{name: 0}) == -1 and b"positive" in lib.vdr_last_error(None), name
    for bad in (0, -4, 32, 5):  # not positive, above p, no divisor of p
        assert call(stride=bad) == -1 and b"stride" in lib.vdr_last_error(None), bad
    for kw in (dict(H=8), dict(Wd=12), dict(H=36), dict(Wd=44)):  # below p; (side - p) no multiple of the stride
        assert call(**kw) == -1 and b"multiples of stride" in lib.vdr_last_error(None), kw


def test_host_refusals_without_an_engine():
    import vdr
    from vdr.engine import Engine
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.set_patch_stride(8)
    e = Engine.__new__(Engine)
    e.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        e.set_patch_stride(8)
    e.cfg = vdr.VdrConfig(img=0, patch=0, in_chans=0, dim=64, heads=1, layers=1, mlp_hidden=128, pre_ln=False, has_pos=False)
    with pytest.raises(ValueError, match="token model"):
        e.set_patch_stride(8)
    e.cfg = vdr.VdrConfig(img=64, patch=16, dim=128, heads=2, layers=1, mlp_hidden=256, has_pos=False, n_register=4, rope=True)
    with pytest.raises(ValueError, match="RoPE"):
        e.set_patch_stride(8)
    e.cfg = vdr.ARCHS["vit_base16_224"]
    for bad in (0, -8, 32, 5, 12):
        with pytest.raises(ValueError, match="divisor of patch 16"):
            e.set_patch_stride(bad)


def test_load_model_refuses_a_stride_on_sam_by_the_models_message(monkeypatch):
    """load_model(..., stride=) hands the stride to VitDescriptorModel.set_patch_stride: its ValueError comes through"""
    import vdr
    from vdr import model as vm

    class Stub:
        def __init__(self, cfg, *a, **k):
            self.cfg = cfg
        set_patch_stride = vm.VitDescriptorModel.set_patch_stride
    monkeypatch.setattr(vm, "VitDescriptorModel", Stub)
    with pytest.raises(ValueError, match="SAM"):
        vm.load_model("medsam", weights={}, stride=8)
    assert isinstance(vm.load_model("medsam", weights={}), Stub)  # (stride=None: nothing is set)


@pytest.mark.parametrize("size,p,s,reg,grid", [((224, 224), 16, 16, 0, (14, 14)), ((224, 224), 16, 8, 0, (27, 27)),
                                               ((224, 224), 16, 4, 0, (53, 53)), ((512, 512), 16, 8, 0, (63, 63)),
                                               ((224, 224), 14, 7, 4, (31, 31)), ((224, 448), 14, 7, 4, (31, 63)),
                                               ((96, 160), 16, 8, 0, (11, 19)), ((160, 96), 16, 2, 0, (73, 41)),
                                               ((64, 96), 32, 8, 0, (5, 9)), ((24, 40), 8, 4, 0, (5, 9))])
def test_grid_arithmetic(size, p, s, reg, grid):
    import vdr
    from vdr.engine import Engine
    e = Engine.__new__(Engine)
    e.cfg = vdr.VdrConfig(img=size[0], patch=p, dim=64, heads=1, layers=1, mlp_hidden=128, n_register=reg)
    assert e.patch_stride == p and e.grid == (size[0] // p, size[0] // p)  # never told a stride: today's geometry
    e._size, e._stride = size, s
    assert e.patch_stride == s and e.grid == grid == sr.grid(size, p, s)
    assert e.n_patches == grid[0] * grid[1] and e.n_tokens == grid[0] * grid[1] + 1 + reg
    with pytest.raises(ValueError, match=rf"images must be \[B,3,{size[0]},{size[1]}\]"):
        e.forward(torch.zeros(1, 3, size[0] + p, size[1]))


@pytest.mark.parametrize("kw", [dict(), dict(act="swiglu", layerscale=True), dict(input_ln=True), dict(has_cls=False)])
def test_restatement_at_stride_p_is_the_oracle(kw):
    """exactly: dyadic pixels (k / 8, k < 8) and integer patch weights and biases make every patch-embedding sum exact in
    fp32 whatever order conv2d and the oracle's im2col GEMM add in (|sum| < 2^24 / 8); the rest is the oracle's own code"""
    cfg = vo.VitCfg(56, 14, 3, 64, 2, 2, 128, **kw)
    w = vo.make_weights(cfg, seed=2, scale=0.05)
    gen = torch.Generator().manual_seed(5)
    w["patch_embed.proj.weight"] = torch.randint(-2, 3, w["patch_embed.proj.weight"].shape, generator=gen).float()
    w["patch_embed.proj.bias"] = torch.randint(-3, 4, (cfg.dim,), generator=gen).float()
    x = torch.randint(0, 8, (3, 3, 56, 56), generator=gen).float() / 8
    for emu in (False, True):
        want = vo.forward_images(cfg, w, x, emulate_bf16=emu)
        got = sr.forward_images(cfg, w, x, cfg.patch, emulate_bf16=emu)
        assert got["grid"] == (4, 4)
        for key in ("patch_embed", "tokens", "cls", "dense"):
            assert torch.equal(got[key], want[key]), (key, emu)


def test_restatement_position_rule_and_overlap():
    """interp_pos is vdr.weights.interpolate_pos_embed (the rule vdr_set_input_size is tested against); a stride-s patch
    embedding holds the stride-p one at every (p/s)-th row and column"""
    from vdr.weights import interpolate_pos_embed
    pos = torch.randn(1, 1 + 16, 32, generator=torch.Generator().manual_seed(0))
    for g in ((7, 7), (4, 4), (5, 11)):
        assert torch.equal(sr.interp_pos(pos, g, 1), interpolate_pos_embed(pos, g, 1))
    assert sr.interp_pos(pos, (4, 4), 1) is pos
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (2, 3, 32, 48), generator=gen).float()
    W = torch.randint(-2, 3, (16, 3, 16, 16), generator=gen).float()
    b = torch.randint(-3, 4, (16,), generator=gen).float()
    fine = sr.patch_embed(x, W, b, 4).reshape(2, 5, 9, 16)
    coarse = sr.patch_embed(x, W, b, 16).reshape(2, 2, 3, 16)
    assert torch.equal(fine[:, ::4, ::4], coarse)
