"""CPU: the SAM / MedSAM encoder at other input sizes (resampled position tables) at the boundary -- declarations,
bindings and exports, refusals that happen before a device is touched, the host-side refusals, the float64 host
definition of the rel-pos resampling (vdr.weights.interpolate_rel_pos, segment_anything's get_rel_pos), and the
definition the device path is tested against: the UNCHANGED oracle fed host-resampled tables reproduces
transformers' SamVisionModel built at other sizes with the native-length tables swapped in
(tests/golden/make_golden_sam_resize.py) to the tolerance of the existing cross-check (1e-4; measured <= 4.3e-6)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import sam_oracle as so
from sam_size_ref import golden_cases, linear_def, within_half_ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_declarations_bindings_and_exports():
    import vdr
    from vdr import _lib, ops, prep, weights
    hdr = _header()
    decl = "int vdr_op_interpolate_rel_pos(const float* table, int L0, int D, float* out, int L, void* stream);"
    assert decl in hdr
    _P, _I = C.c_void_p, C.c_int
    assert _lib.SYMBOLS["vdr_op_interpolate_rel_pos"] == (_I, [_P, _I, _I, _P, _I, _P])
    assert hasattr(_lib.load(), "vdr_op_interpolate_rel_pos")
    # additive: no ABI bump, vdr_config keeps its layout
    assert _lib.load().vdr_abi_version() == 8 and "#define VDR_ABI_VERSION 8" in hdr
    assert C.sizeof(_lib.vdr_config) == 100
    assert callable(ops.interpolate_rel_pos) and callable(weights.interpolate_rel_pos)
    import inspect
    assert list(inspect.signature(prep.prepare_image).parameters) == ["img", "side", "device"]
    assert inspect.signature(vdr.load_model).parameters["img_size"].default is None


def test_refusals_before_a_device():
    from vdr import _lib
    lib = _lib.load()
    b = (C.c_char * 64)()
    ok = dict(table=b, L0=3, D=4, out=b, L=5)

    def call(**kw):
        a = {**ok, **kw}
        return lib.vdr_op_interpolate_rel_pos(a["table"], a["L0"], a["D"], a["out"], a["L"], None)
    for name in ("table", "out"):
        assert call(**{name: None}) == -1, name  # VDR_ERR_INVALID
        assert name.encode() in lib.vdr_last_error(None) and b"null" in lib.vdr_last_error(None)
    for name in ("L0", "D", "L"):
        for bad in (0, -3):
            assert call(**{name: bad}) == -1, (name, bad)
            assert re.search(rb"\b" + name.encode() + rb"\b", lib.vdr_last_error(None)), (name, lib.vdr_last_error(None))
    # attention over a grid side above 64: refused with VDR_ERR_UNSUPPORTED and a message that says so
    assert lib.vdr_op_attention_relpos(b, b, b, b, b, 1, 65, 1, None) == -7
    assert b"64" in lib.vdr_last_error(None)
    # vdr_create: a SAM configuration with global blocks over a grid side above 64
    import vdr
    h = C.c_void_p()
    cc = vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "img": 1040}).to_c()
    assert lib.vdr_create(C.byref(cc), 0, C.byref(h)) == -7
    msg = lib.vdr_last_error(None)
    assert b"65" in msg and b"at most 64" in msg, msg
    # ... and one whose side is no multiple of the patch side (VDR_ERR_INVALID, as for every image model)
    cc = vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "img": 520}).to_c()
    assert lib.vdr_create(C.byref(cc), 0, C.byref(h)) == -1


def test_host_refusals_without_an_engine():
    import vdr
    from vdr import ops
    for bad, what in ((1040, "at most 64"), ((512, 256), "square"), (520, "multiple of the patch"), (0, "multiple of the patch"),
                      (-512, "multiple of the patch")):
        with pytest.raises(ValueError, match=what):
            vdr.load_model("medsam", weights={}, img_size=bad)
    with pytest.raises(ValueError, match="SAM"):
        vdr.load_model("vit_base16_224", weights={}, img_size=448)  # plain ViTs change size with set_input_size
    with pytest.raises(ValueError, match="1..64"):
        ops.attention_relpos(torch.zeros(1), torch.zeros(1), torch.zeros(1), 1, 65, 1)
    from vdr.model import sam_input_side
    assert sam_input_side(512, 16) == 512 and sam_input_side((256, 256), 16) == 256 and sam_input_side(1024, 16) == 1024
    # the size of a SAM model stays a load-time property
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.VdrConfig(**{**vdr.ARCHS["medsam"].__dict__, "img": 512})
    with pytest.raises(ValueError, match="SAM"):
        m.set_input_size(256, 256)


def test_interpolate_rel_pos_host_definition():
    from vdr.weights import interpolate_rel_pos
    gen = torch.Generator().manual_seed(5)
    # exact on integer tables where every weight is dyadic: L0 / L = 2 (weights 1/2), 4 (1/2), 1/2 (1/4, 3/4), 1/4 (eighths)
    for L0, L in ((26, 13), (28, 7), (8, 16), (5, 20)):
        t = torch.randint(-64, 64, (L0, 8), generator=gen).float()
        got = interpolate_rel_pos(t, L)
        want = linear_def(t, L)
        assert got.dtype == torch.float32 and got.shape == (L, 8)
        assert np.array_equal(got.numpy().astype(np.float64), want), (L0, L)
    # downsampling by 2 averages neighbouring rows; upsampling keeps the end rows (clamped neighbours)
    t = torch.arange(12.0).reshape(6, 2)
    assert torch.equal(interpolate_rel_pos(t, 3), torch.tensor([[1.0, 2.0], [5.0, 6.0], [9.0, 10.0]]))
    up = interpolate_rel_pos(t, 12)
    assert torch.equal(up[0], t[0]) and torch.equal(up[-1], t[-1])
    # random tables at the SAM lengths 2 g - 1: F.interpolate in fp32 to fp32 rounding (of its source coordinate), the float64 definition to one rounding
    for g0, g in ((14, 9), (14, 20), (64, 32), (64, 16), (64, 48), (10, 15), (7, 64)):
        t = torch.randn(2 * g0 - 1, 64, generator=gen)
        got = interpolate_rel_pos(t, 2 * g - 1)
        f32 = torch.nn.functional.interpolate(t.t().unsqueeze(0), size=2 * g - 1, mode="linear", align_corners=False)[0].t()
        # torch's fp32 path rounds the source coordinate (magnitude < L0, three operations: 3 * 2^-24 * L0 absolute), which
        # moves the weight by as much and the result by that times |t[i1] - t[i0]| <= 2 max|t|; plus the fp32 blend itself
        tmax, L0 = float(t.abs().max()), 2 * g0 - 1
        assert float((got - f32).abs().max()) <= (3 * 2.0 ** -24 * L0) * 2 * tmax + 4 * 2.0 ** -24 * tmax, (g0, g)
        want = linear_def(t, 2 * g - 1)
        assert within_half_ulp(got, want), (g0, g)
    # identity at L == L0: the table itself
    t = torch.randn(27, 64, generator=gen)
    assert torch.equal(interpolate_rel_pos(t, 27), t)
    with pytest.raises(ValueError):
        interpolate_rel_pos(t, 0)
    with pytest.raises(ValueError):
        interpolate_rel_pos(torch.zeros(3), 5)


def test_sam_tables_at_resamples_only_what_depends_on_the_grid():
    from vdr.weights import interpolate_pos_embed, interpolate_rel_pos, sam_tables_at
    cfg = so.SamCfg(224, 16, 3, 64, 1, 3, 128, 7, (1,), 64, 1e-6)
    w = so.make_weights(cfg, seed=3)
    ws = sam_tables_at(w, 9, cfg.global_idx)
    assert tuple(ws["pos_embed"].shape) == (1, 9, 9, 64)
    assert torch.equal(ws["pos_embed"].reshape(1, 81, 64), interpolate_pos_embed(w["pos_embed"].reshape(1, 196, 64), (9, 9), 0))
    assert torch.equal(ws["blocks.1.attn.rel_pos_h"], interpolate_rel_pos(w["blocks.1.attn.rel_pos_h"], 17))
    for k in w:
        if k != "pos_embed" and not k.startswith("blocks.1.attn.rel_pos"):
            assert ws[k] is w[k], k  # window tables [2 window - 1, 64] included
    same = sam_tables_at(w, 14, cfg.global_idx)
    assert all(torch.equal(same[k], w[k]) for k in w)


def test_oracle_with_host_resampled_tables_reproduces_transformers(golden_dir):
    from vdr.weights import sam_tables_at
    cases = golden_cases(golden_dir)
    sides = sorted((c[0].img, c[1].img, c[0].window) for c in cases)
    for need in ((224, 64, 7), (224, 112, 7), (224, 144, 7), (224, 192, 7), (224, 320, 7), (160, 96, 4), (160, 240, 4)):
        assert need in sides, need
    for cn, cs, batch, wseed, xseed, wscale, want in cases:
        w0 = so.make_weights(cn, seed=wseed, scale=wscale)
        x = so.make_images(cs, batch, seed=xseed)
        out = so.sam_forward(cs, sam_tables_at(w0, cs.grid, cs.global_idx), x)["out"][:, :want.shape[1]]
        err = float((out - want).abs().max())
        print(f"{cn.img} -> {cs.img}: max |oracle - transformers| = {err:.3e}")
        assert err <= 1e-4, (cn.img, cs.img, err)
        # the fixture sees a wrong rule: centre-cropped / zero-padded tables instead of resampled ones
        if cs.grid < cn.grid:
            wrong = dict(sam_tables_at(w0, cs.grid, cs.global_idx))
            for i in cs.global_idx:
                for ax in "hw":
                    k = f"blocks.{i}.attn.rel_pos_{ax}"
                    o = (w0[k].shape[0] - (2 * cs.grid - 1)) // 2
                    wrong[k] = w0[k][o:o + 2 * cs.grid - 1].clone()
            bad = float((so.sam_forward(cs, wrong, x)["out"][:, :want.shape[1]] - want).abs().max())
            assert bad > 1e-3, (cn.img, cs.img, bad)
