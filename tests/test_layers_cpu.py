"""CPU: vdr_forward_layers (intermediate-layer and mean-pooled outputs) is declared, bound and laid out as the header says,
refuses bad arguments before it touches a device, and the host-side block resolution of get_intermediate_layers follows
DINOv2's."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")


def test_header_and_binding_declare_forward_layers():
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"int vdr_forward_layers\(vdr_handle h, const void\* images, int in_dtype, int batch,\s*"
                     r"const vdr_layer_out\* outs, int n_outs,\s*void\* workspace, size_t workspace_bytes, void\* stream\);", src)
    assert re.search(r"VDR_OUT_POOLED = 5\b", src)
    assert "} vdr_layer_out;" in src
    assert "vdr_forward_layers" in _lib.SYMBOLS
    assert _lib.OUT_POOLED == 5
    lib = _lib.load()
    assert hasattr(lib, "vdr_forward_layers")
    assert lib.vdr_abi_version() == 8


def test_layer_out_struct_layout_matches_header():
    from vdr import _lib
    # four int32, one int64, one pointer: 32 bytes, ld at offset 16, out at 24
    assert C.sizeof(_lib.vdr_layer_out) == 32
    assert _lib.vdr_layer_out.ld.offset == 16 and _lib.vdr_layer_out.out.offset == 24
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} vdr_layer_out;", src).group(1)
    fields = re.findall(r"(\w+\*?)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.vdr_layer_out._fields_]
    assert [t for t, _ in fields] == ["int32_t"] * 4 + ["int64_t", "void*"]


def _call(lib, outs, n=None, handle=None):
    arr = (type(outs[0]) * len(outs))(*outs) if outs else None
    buf = (C.c_char * 64)()
    return lib.vdr_forward_layers(handle, buf, 0, 2, arr, len(outs) if n is None else n, buf, 64, None)


def test_forward_layers_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def out(**kw):
        o = _lib.vdr_layer_out(layer=0, out_mode=_lib.OUT_CLS, out_dtype=_lib.VDR_F32, norm=1, ld=0, out=ptr)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    # null outs / n_outs <= 0
    assert lib.vdr_forward_layers(None, buf, 0, 2, None, 1, buf, 64, None) == -1
    assert b"outs" in lib.vdr_last_error(None)
    assert _call(lib, [out()], n=0) == -1
    assert _call(lib, [out()], n=-3) == -1
    # per-output refusals (checked before the handle): message names the field
    cases = [
        (dict(out=None), b"null out"),
        (dict(out_mode=_lib.OUT_PATCH_EMBED), b"out_mode"),
        (dict(out_mode=_lib.OUT_ENCODER), b"out_mode"),
        (dict(out_mode=6), b"out_mode"),
        (dict(out_mode=-1), b"out_mode"),
        (dict(out_dtype=_lib.VDR_F64), b"out_dtype"),
        (dict(out_dtype=7), b"out_dtype"),
        (dict(norm=2), b"norm"),
        (dict(ld=-1), b"ld"),
        (dict(out_mode=_lib.OUT_DENSE, ld=1024), b"ld must be 0"),
        (dict(out_mode=_lib.OUT_TOKENS, ld=768), b"ld must be 0"),
    ]
    for kw, msg in cases:
        assert _call(lib, [out(), out(**kw)]) == -1, kw  # VDR_ERR_INVALID
        err = lib.vdr_last_error(None)
        assert msg in err and b"outs[1]" in err, (kw, err)
    # every output well-formed: the null handle itself is refused
    assert _call(lib, [out(), out(out_mode=_lib.OUT_POOLED, ld=4000), out(out_mode=_lib.OUT_DENSE, norm=0)]) == -1
    assert b"null" in lib.vdr_last_error(None)


def test_forward_still_refuses_the_pooled_mode():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    assert lib.vdr_forward(None, buf, 0, 1, buf, _lib.OUT_POOLED, 0, buf, 64, None) == -1


def test_intermediate_layer_indices_follow_dinov2():
    from vdr.model import intermediate_layer_indices as idx
    assert idx(1, 12) == [11]
    assert idx(4, 12) == [8, 9, 10, 11]
    assert idx(12, 12) == list(range(12))
    assert idx([0, 5, 11], 12) == [0, 5, 11]
    assert idx((11, 2), 12) == [2, 11]  # DINOv2 visits the blocks in order: the result is in block order
    assert idx(range(3), 4) == [0, 1, 2]
    for bad in (0, 13, -1, [12], [-1], [3, 3], [], True):
        with pytest.raises(ValueError):
            idx(bad, 12)


def test_model_methods_refuse_sam_models_on_the_host():
    """The SAM check needs no device: it is the first thing both methods do."""
    import vdr
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.get_intermediate_layers(None, 4)
    with pytest.raises(ValueError, match="SAM"):
        m.linear_probe_features(None)
    m.cfg = vdr.ARCHS["dinov2"]  # patch embedding only: no blocks
    with pytest.raises(ValueError, match="no transformer blocks"):
        m.get_intermediate_layers(None, 1)
