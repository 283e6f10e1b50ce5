"""CPU: facet descriptors and log-binning -- the two fp32 restatements of the log-bin (tests/descriptor_ref.py) agree, the
new entry points (vdr_op_log_bin, vdr_forward_facets) are declared, bound, exported and laid out as the header says and
refuse bad arguments before they touch a device, the Python surface refuses what it must on the host, and the
transformers golden (tests/golden/vit_hf_facets.npz) loads and is met by the fp32 facet restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import descriptor_ref as dref
from oracle import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")
GRIDS = ((1, 1), (2, 3), (7, 5), (10, 11))
HIERARCHIES = (1, 2, 3)


def _designed(gen, B, n, C):
    """integer values, |v| <= 64: every fp32 window sum (at most 81 terms) is exact"""
    return torch.randint(-64, 65, (B, n, C), generator=gen).float()


@pytest.mark.parametrize("h", HIERARCHIES)
@pytest.mark.parametrize("grid", GRIDS)
def test_the_two_log_bin_restatements_agree_bitwise_on_integer_inputs(grid, h):
    gh, gw = grid
    gen = torch.Generator().manual_seed(100 * gh + 10 * gw + h)
    x = _designed(gen, 2, gh * gw, 8)
    a = dref.log_bin_brute(x, gh, gw, h)
    b = dref.log_bin_pool(x, gh, gw, h).numpy()
    assert a.shape == (2, gh * gw, (1 + 8 * h) * 8) and a.dtype == np.float32
    assert np.array_equal(a, b)
    # level 0: the patch itself is bin 4, the other eight are its clamped neighbours
    assert np.array_equal(a[:, :, 4 * 8:5 * 8], x.numpy())


@pytest.mark.parametrize("h", HIERARCHIES)
@pytest.mark.parametrize("grid", GRIDS)
def test_the_two_log_bin_restatements_agree_within_the_summation_bound_on_random_inputs(grid, h):
    gh, gw = grid
    gen = torch.Generator().manual_seed(7 + 100 * gh + 10 * gw + h)
    x = torch.randn(2, gh * gw, 16, generator=gen).to(torch.bfloat16).float()
    a = dref.log_bin_brute(x, gh, gw, h)
    b = dref.log_bin_pool(x, gh, gw, h).numpy()
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    bound = dref.log_bin_bound(x, h, a)
    assert (err <= bound).all(), (grid, h, float(err.max()), float((err - bound).max()))
    assert np.array_equal(a[:, :, :9 * 16], b[:, :, :9 * 16])  # level 0: copies


def test_bin_order_and_count():
    assert dref.bin_offsets(1) == [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    for h in HIERARCHIES:
        o = dref.bin_offsets(h)
        assert len(o) == 1 + 8 * h
        assert [k for k, _, _ in o] == [0] * 9 + [k for k in range(1, h) for _ in range(8)]
    assert dref.bin_offsets(2)[9:] == [(1, dy, dx) for dy in (-3, 0, 3) for dx in (-3, 0, 3) if (dy, dx) != (0, 0)]


def test_header_binding_and_exports_declare_the_descriptor_entry_points():
    import vdr
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"int vdr_op_log_bin\(const void\* x, int in_dtype, int64_t ld, int64_t image_stride, int batch, int gh, int gw, "
                     r"int C,\s*int hierarchy, float\* work, void\* out, int out_dtype, void\* stream\);", src)
    assert re.search(r"int vdr_forward_facets\(vdr_handle h, const void\* images, int in_dtype, int batch, const vdr_layer_out\* outs, "
                     r"int n_outs,\s*const vdr_attn_map\* maps, int n_maps, const vdr_facet_out\* facets, int n_facets, "
                     r"void\* workspace,\s*size_t workspace_bytes, void\* stream\);", src)
    assert "} vdr_facet_out;" in src
    assert re.search(r"enum \{ VDR_FACET_TOKEN = 0, VDR_FACET_QUERY = 1, VDR_FACET_KEY = 2, VDR_FACET_VALUE = 3 \};", src)
    assert re.search(r"#define VDR_ABI_VERSION 8\b", src)
    for name in ("vdr_op_log_bin", "vdr_forward_facets"):
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_log_bin") and hasattr(lib, "vdr_forward_facets")
    assert lib.vdr_abi_version() == 8
    assert (_lib.FACET_TOKEN, _lib.FACET_QUERY, _lib.FACET_KEY, _lib.FACET_VALUE) == (0, 1, 2, 3)
    assert vdr.FacetOut is vdr.engine.FacetOut
    assert [f.name for f in vdr.FacetOut.__dataclass_fields__.values()] == ["layer", "facet", "hierarchy", "all_rows", "dtype", "out"]
    from vdr import ops
    from vdr.model import VitDescriptorModel
    assert callable(ops.log_bin) and callable(vdr.Engine.forward_descriptors) and callable(VitDescriptorModel.extract_descriptors)


def test_facet_out_struct_layout_matches_header():
    from vdr import _lib
    # five int32 (20 bytes), padding to the pointer's alignment, one pointer: 32 bytes, out at offset 24
    assert C.sizeof(_lib.vdr_facet_out) == 32
    assert _lib.vdr_facet_out.out.offset == 24
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} vdr_facet_out;", src).group(1)
    fields = re.findall(r"(\w+\*?)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.vdr_facet_out._fields_]
    assert [t for t, _ in fields] == ["int32_t"] * 5 + ["void*"]
    # the structs that were there keep their size
    assert C.sizeof(_lib.vdr_attn_map) == 24 and C.sizeof(_lib.vdr_layer_out) == 32


def test_op_log_bin_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 4096)()
    base = (C.addressof(raw) + 255) & ~255
    x, work, out = base, base + 1024, base + 2048
    BF, F32 = _lib.VDR_BF16, _lib.VDR_F32

    def call(x=x, in_dtype=BF, ld=8, image_stride=48, batch=1, gh=2, gw=3, Cc=8, h=2, work=work, out=out, out_dtype=F32):
        return lib.vdr_op_log_bin(x, in_dtype, ld, image_stride, batch, gh, gw, Cc, h, work, out, out_dtype, None)

    for h in (0, -1, 4, 9):
        assert call(h=h) == -7, h  # VDR_ERR_UNSUPPORTED
        assert b"hierarchy" in lib.vdr_last_error(None)
    invalid = [dict(Cc=4), dict(Cc=12), dict(Cc=0), dict(ld=7), dict(Cc=16, ld=8), dict(x=None), dict(out=None), dict(work=None),
               dict(batch=0), dict(gh=0), dict(gw=-1), dict(x=x + 2), dict(x=x + 8), dict(out=out + 4), dict(work=work + 4),
               dict(ld=12), dict(image_stride=52), dict(in_dtype=F32, ld=10), dict(in_dtype=2), dict(out_dtype=3)]
    for kw in invalid:
        assert call(**kw) == -1, kw  # VDR_ERR_INVALID
    # (h == 1 needs no work buffer: with one, the well-formed call gets as far as the device check or the launch)
    assert call(h=1, work=None) in (0, -2, -3)


def test_forward_facets_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def facet(**kw):
        f = _lib.vdr_facet_out(layer=0, facet=_lib.FACET_KEY, hierarchy=0, all_rows=0, out_dtype=_lib.VDR_F32, out=ptr)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def call(facets, n=None, outs=None, n_outs=0, maps=None, n_maps=0):
        arr = (_lib.vdr_facet_out * len(facets))(*facets) if facets else None
        return lib.vdr_forward_facets(None, buf, 0, 2, outs, n_outs, maps, n_maps, arr, len(facets) if n is None else n, buf, 64, None)

    assert call([]) == -1
    assert b"facets" in lib.vdr_last_error(None)
    assert call([facet()], n=0) == -1
    cases = [(dict(out=None), b"null out"), (dict(facet=4), b"facet"), (dict(facet=-1), b"facet"), (dict(hierarchy=4), b"hierarchy"),
             (dict(hierarchy=-1), b"hierarchy"), (dict(all_rows=2), b"all_rows"), (dict(all_rows=1, hierarchy=2), b"all_rows"),
             (dict(out_dtype=_lib.VDR_F64), b"out_dtype")]
    for kw, msg in cases:
        assert call([facet(), facet(**kw)]) == -1, kw
        err = lib.vdr_last_error(None)
        assert msg in err and b"facets[1]" in err, (kw, err)
    # outs and maps keep their checks
    bad_out = _lib.vdr_layer_out(layer=0, out_mode=6, out_dtype=_lib.VDR_F32, norm=1, ld=0, out=ptr)
    assert call([facet()], outs=(_lib.vdr_layer_out * 1)(bad_out), n_outs=1) == -1
    assert b"outs[0]" in lib.vdr_last_error(None)
    bad_map = _lib.vdr_attn_map(layer=0, q_rows=0, head_mean=0, out_dtype=_lib.VDR_F32, out=ptr)
    assert call([facet()], maps=(_lib.vdr_attn_map * 1)(bad_map), n_maps=1) == -1
    assert b"maps[0]" in lib.vdr_last_error(None)
    assert call([facet()], n_outs=1) == -1 and call([facet()], n_maps=-1) == -1
    # well-formed facets: the null handle itself is refused
    assert call([facet(), facet(facet=_lib.FACET_TOKEN, all_rows=1, out_dtype=_lib.VDR_BF16), facet(hierarchy=3)]) == -1
    assert b"null" in lib.vdr_last_error(None)


def test_python_refusals_need_no_device():
    import vdr
    from vdr import pipeline
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["vit_tiny16_224"]
    m.model_name = "vit_tiny16_224"
    with pytest.raises(ValueError, match="facet"):
        m.extract_descriptors(None, facet="keys")
    with pytest.raises(ValueError, match="include_cls"):
        m.extract_descriptors(None, bin=True, include_cls=True)
    for h in (0, 4, -1):
        with pytest.raises(ValueError, match="hierarchy"):
            m.extract_descriptors(None, bin=True, hierarchy=h)
    with pytest.raises(ValueError, match="reshape"):
        m.extract_descriptors(None, include_cls=True, reshape=True)
    with pytest.raises(ValueError, match="out of range"):
        m.extract_descriptors(None, layer=12)
    with pytest.raises(ValueError, match="facet"):
        vdr.get_dense_descriptor(m, np.zeros((8, 8, 3), np.float32), facet="attn")
    with pytest.raises(ValueError, match="hierarchy"):
        vdr.extract_dense(m, None, facet="key", bin=True, hierarchy=5)
    with pytest.raises(ValueError, match="facet"):
        pipeline.generate_features(m, None, None, descriptor={"facet": "nope"})
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.generate_features(m, None, None, descriptor={"include_cls": True})
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.extract_descriptors(None)
    with pytest.raises(ValueError, match="SAM"):
        pipeline.generate_features(m, None, None, descriptor={"facet": "key"})
    m.cfg = vdr.ARCHS["dinov2"]  # patch embedding only: no blocks
    with pytest.raises(ValueError, match="no blocks"):
        m.extract_descriptors(None, facet="token")
    with pytest.raises(ValueError, match="facet"):
        vdr.engine.check_facet("k", 0, False)


def test_golden_loads_and_the_fp32_restatement_meets_it(golden_dir):
    g = np.load(os.path.join(golden_dir, "vit_hf_facets.npz"), allow_pickle=False)
    cfg = vo.VitCfg(int(g["img"]), int(g["patch"]), 3, int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"]))
    assert cfg.layers == 2
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = vo.make_images(cfg, int(g["batch"]), seed=int(g["xseed"]))
    ref = dref.facets(dref.plain(cfg), w, x)
    for f in ("query", "key", "value", "token"):
        for i in range(cfg.layers):
            want = torch.from_numpy(g[f"{f}.{i}"])
            assert want.shape == (int(g["batch"]), cfg.n_tokens, cfg.dim)
            err = float((ref[f][i] - want).abs().max())
            assert err <= 2.5e-6, (f, i, err)
    # token of the last block through the final norm is vit_hf_tiny's stored output: one network, two goldens
    tiny = np.load(os.path.join(golden_dir, "vit_hf_tiny.npz"), allow_pickle=False)
    last = vo.layer_norm(torch.from_numpy(g["token.1"]), w["norm.weight"], w["norm.bias"], cfg.ln_eps)
    assert float((last - torch.from_numpy(tiny["tokens"])).abs().max()) <= 2.5e-6
