"""CPU: the attention-map entry points (vdr_op_attention_probs, vdr_forward_attn_maps) are declared, bound, exported and
laid out as the header says, refuse bad arguments before they touch a device, and the Python methods refuse the models
that have no such maps on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")


def test_header_binding_and_exports_declare_the_attention_map_entry_points():
    import vdr
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"int vdr_op_attention_probs\(const void\* qkv, void\* out, int batch, int seq, int heads, int head_dim, "
                     r"int q_rows,\s*int head_mean, int out_dtype, void\* stream\);", src)
    assert re.search(r"int vdr_forward_attn_maps\(vdr_handle h, const void\* images, int in_dtype, int batch, "
                     r"const vdr_layer_out\* outs, int n_outs,\s*const vdr_attn_map\* maps, int n_maps, void\* workspace, "
                     r"size_t workspace_bytes, void\* stream\);", src)
    assert "} vdr_attn_map;" in src
    assert re.search(r"#define VDR_ABI_VERSION 8\b", src)
    for name in ("vdr_op_attention_probs", "vdr_forward_attn_maps"):
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_attention_probs") and hasattr(lib, "vdr_forward_attn_maps")
    assert lib.vdr_abi_version() == 8
    assert vdr.AttnMap is vdr.engine.AttnMap
    assert [f.name for f in vdr.AttnMap.__dataclass_fields__.values()] == ["layer", "q_rows", "head_mean", "dtype", "out"]
    from vdr import ops
    assert callable(ops.attention_probs)
    from vdr.model import VitDescriptorModel
    assert callable(VitDescriptorModel.get_last_selfattention) and callable(VitDescriptorModel.get_attention_maps)


def test_attn_map_struct_layout_matches_header():
    from vdr import _lib
    # four int32 and one pointer: 24 bytes, out at offset 16
    assert C.sizeof(_lib.vdr_attn_map) == 24
    assert _lib.vdr_attn_map.out.offset == 16
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} vdr_attn_map;", src).group(1)
    fields = re.findall(r"(\w+\*?)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.vdr_attn_map._fields_]
    assert [t for t, _ in fields] == ["int32_t"] * 4 + ["void*"]


def test_forward_attn_maps_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def amap(**kw):
        a = _lib.vdr_attn_map(layer=0, q_rows=1, head_mean=0, out_dtype=_lib.VDR_F32, out=ptr)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(maps, n=None, outs=None, n_outs=0):
        arr = (_lib.vdr_attn_map * len(maps))(*maps) if maps else None
        return lib.vdr_forward_attn_maps(None, buf, 0, 2, outs, n_outs, arr, len(maps) if n is None else n, buf, 64, None)

    # null maps / n_maps <= 0
    assert call([]) == -1
    assert b"maps" in lib.vdr_last_error(None)
    assert call([amap()], n=0) == -1
    assert call([amap()], n=-2) == -1
    # per-map refusals, ahead of the handle check: the message names maps[k] and the field
    cases = [
        (dict(out=None), b"null out"),
        (dict(q_rows=0), b"q_rows"),
        (dict(q_rows=-5), b"q_rows"),
        (dict(head_mean=2), b"head_mean"),
        (dict(head_mean=-1), b"head_mean"),
        (dict(out_dtype=_lib.VDR_F64), b"out_dtype"),
        (dict(out_dtype=7), b"out_dtype"),
    ]
    for kw, msg in cases:
        assert call([amap(), amap(**kw)]) == -1, kw  # VDR_ERR_INVALID
        err = lib.vdr_last_error(None)
        assert msg in err and b"maps[1]" in err, (kw, err)
    # the outs keep vdr_forward_layers' checks and messages
    bad_out = _lib.vdr_layer_out(layer=0, out_mode=6, out_dtype=_lib.VDR_F32, norm=1, ld=0, out=ptr)
    assert call([amap()], outs=(_lib.vdr_layer_out * 1)(bad_out), n_outs=1) == -1
    err = lib.vdr_last_error(None)
    assert b"out_mode" in err and b"outs[0]" in err
    assert call([amap()], outs=None, n_outs=1) == -1
    assert call([amap()], outs=None, n_outs=-1) == -1
    # every map well-formed, no outs: the null handle itself is refused
    assert call([amap(), amap(layer=3, q_rows=100000, head_mean=1, out_dtype=_lib.VDR_BF16)]) == -1
    assert b"null" in lib.vdr_last_error(None)


def test_forward_layers_keeps_its_refusals():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value
    o = _lib.vdr_layer_out(layer=0, out_mode=6, out_dtype=_lib.VDR_F32, norm=1, ld=0, out=ptr)
    assert lib.vdr_forward_layers(None, buf, 0, 2, (_lib.vdr_layer_out * 1)(o), 1, buf, 64, None) == -1
    assert lib.vdr_last_error(None) == b"outs[0]: out_mode must be CLS, DENSE, TOKENS or POOLED"
    assert lib.vdr_forward_layers(None, buf, 0, 2, None, 1, buf, 64, None) == -1
    assert lib.vdr_last_error(None) == b"null outs or n_outs <= 0"


def test_op_attention_probs_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    for dh in (0, 16, 48, 63, 65, 256):
        assert lib.vdr_op_attention_probs(buf, buf, 1, 8, 2, dh, 1, 0, 0, None) == -7, dh  # VDR_ERR_UNSUPPORTED
        assert b"head dim" in lib.vdr_last_error(None)
    assert lib.vdr_op_attention_probs(None, buf, 1, 8, 2, 64, 1, 0, 0, None) == -1
    assert lib.vdr_op_attention_probs(buf, None, 1, 8, 2, 64, 1, 0, 0, None) == -1
    assert b"null" in lib.vdr_last_error(None)
    for q_rows in (0, -1, 9, 100):
        assert lib.vdr_op_attention_probs(buf, buf, 1, 8, 2, 64, q_rows, 0, 0, None) == -1, q_rows
        assert b"q_rows" in lib.vdr_last_error(None)
    assert lib.vdr_op_attention_probs(buf, buf, 1, 8, 2, 64, 1, 2, 0, None) == -1
    assert b"head_mean" in lib.vdr_last_error(None)
    for dt in (2, 3, 7):
        assert lib.vdr_op_attention_probs(buf, buf, 1, 8, 2, 64, 1, 0, dt, None) == -1
        assert b"out_dtype" in lib.vdr_last_error(None)
    for shape in ((0, 8, 2), (1, 0, 2), (1, 8, 0)):
        assert lib.vdr_op_attention_probs(buf, buf, *shape, 64, 1, 0, 0, None) == -1


def test_model_methods_refuse_maps_the_model_does_not_have_on_the_host():
    """SAM (windowed, rel-pos attention), the patch-embedding-only 'dinov2' drop-in and, for cls_only, a model without a
    CLS token are refused before anything runs: no engine, no device."""
    import vdr
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.get_last_selfattention(None)
    with pytest.raises(ValueError, match="SAM"):
        m.get_attention_maps(None)
    m.cfg = vdr.ARCHS["dinov2"]  # patch embedding only: no blocks
    with pytest.raises(ValueError, match="no transformer blocks"):
        m.get_last_selfattention(None)
    with pytest.raises(ValueError, match="no transformer blocks"):
        m.get_attention_maps(None, cls_only=False)
    m.cfg = vdr.VdrConfig(img=64, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, has_cls=False)
    with pytest.raises(ValueError, match="CLS token"):
        m.get_attention_maps(None)
    m.cfg = vdr.ARCHS["vit_tiny16_224"]
    with pytest.raises(ValueError, match="reshape"):
        m.get_attention_maps(None, cls_only=False, reshape=True)
    with pytest.raises(ValueError, match="out of range"):
        m.get_attention_maps(None, layers=[0, 12])
