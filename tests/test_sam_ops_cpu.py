"""CPU: the SAM window-path entry points (vdr_op_layernorm_window, vdr_op_layernorm_mx_window, vdr_op_linear_window,
vdr_op_im2col3) refuse every bad argument before they touch a device, with the codes and texts their sibling ops use, and
fail with VDR_ERR_NO_DEVICE on a box without a GPU; and the row maps tests/test_sam_ops_gpu.py compares the kernels with
(tests/sam_ops_ref.py) are segment_anything's window_partition / window_unpartition (oracle.sam_oracle)."""
import ctypes as C

import pytest
import torch

import sam_ops_ref as sr
from fixtures import lib  # noqa: F401

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -7


@pytest.fixture(scope="module")
def buf():
    raw = (C.c_char * 256)()
    base = (C.addressof(raw) + 15) & ~15  # a 16-byte aligned address inside raw
    return raw, base


def _refused(lib, fn, ok, code, text, **kw):
    a = list(ok)
    for i, v in kw.items():
        a[int(i[1:])] = v
    assert fn(*a) == code, (kw, lib.vdr_last_error(None))
    assert text in lib.vdr_last_error(None), (kw, lib.vdr_last_error(None))


def test_layernorm_window_refusals(lib, buf):
    _, b = buf
    # x, y, gamma, beta, batch, g, ws, D, eps, stream
    ok = [b, b, b, b, 2, 10, 4, 64, 1e-6, None]
    fn = lib.vdr_op_layernorm_window
    for i in range(4):
        _refused(lib, fn, ok, INVALID, b"null argument", **{f"a{i}": None})
    for i in (4, 5, 6):
        for v in (0, -1):
            _refused(lib, fn, ok, INVALID, b"bad shape", **{f"a{i}": v})
    _refused(lib, fn, ok, INVALID, b"2^31 windowed rows", a4=1 << 20, a5=64, a6=14)
    _refused(lib, fn, ok, INVALID, b"2^31 windowed rows", a5=40000)
    for D in (0, -4, 66, 2052, 4096):
        _refused(lib, fn, ok, UNSUPPORTED, b"D must be a positive multiple of 4, at most 2048", a7=D)
    for i in range(4):
        _refused(lib, fn, ok, INVALID, b"16-byte aligned", **{f"a{i}": b + 8})


def test_layernorm_mx_window_refusals(lib, buf):
    _, b = buf
    # x, gamma, beta, eps, batch, g, ws, D, q, scales, stream
    ok = [b, b, b, 1e-6, 2, 10, 4, 64, b, b, None]
    fn = lib.vdr_op_layernorm_mx_window
    for i in (0, 1, 2, 8, 9):
        _refused(lib, fn, ok, INVALID, b"null argument", **{f"a{i}": None})
    for i in (4, 5, 6):
        for v in (0, -1):
            _refused(lib, fn, ok, INVALID, b"bad shape", **{f"a{i}": v})
    _refused(lib, fn, ok, INVALID, b"2^31 windowed rows", a4=1 << 20, a5=64, a6=14)
    for D in (0, -32, 16, 48, 100, 2080):
        _refused(lib, fn, ok, UNSUPPORTED, b"D must be a positive multiple of 32, at most 2048", a7=D)
    for i in (0, 1, 2, 8):
        _refused(lib, fn, ok, INVALID, b"16-byte aligned", **{f"a{i}": b + 8})


def test_linear_window_refusals(lib, buf):
    _, b = buf
    # x, W, bias, resid, y, batch, g, ws, N, K, variant, part, part_stride, stream
    ok = [b, b, b, b, b, 2, 10, 4, 128, 64, 26, None, 0, None]
    fn = lib.vdr_op_linear_window
    for i in (0, 1, 3, 4):
        _refused(lib, fn, ok, INVALID, b"null argument", **{f"a{i}": None})
    for i in (5, 6, 7):
        for v in (0, -1):
            _refused(lib, fn, ok, INVALID, b"bad shape", **{f"a{i}": v})
    _refused(lib, fn, ok, INVALID, b"2^31 windowed rows", a5=1 << 20, a6=64, a7=14)
    # the text vdr_op_linear gives for the same constraints
    for K in (0, -64, 32, 96, 100):
        _refused(lib, fn, ok, UNSUPPORTED, b"K % 64 == 0 and N % 8 == 0 required", a9=K)
    for N in (0, -8, 4, 100, 127):
        _refused(lib, fn, ok, UNSUPPORTED, b"K % 64 == 0 and N % 8 == 0 required", a8=N)
    for v in (-1, 1, 21, 30, 31, 32, 100, 126):
        _refused(lib, fn, ok, INVALID, b"variant", a10=v)
    # the LayerNorm partials: whole 64-column groups and a stride that holds every token row
    for N in (8, 72, 200):
        _refused(lib, fn, ok, INVALID, b"part needs N % 64 == 0", a8=N, a11=b, a12=200)
    _refused(lib, fn, ok, INVALID, b"part_stride >= batch * g * g", a11=b, a12=199)
    for i in (0, 1, 2, 3, 4):
        _refused(lib, fn, ok, INVALID, b"16-byte aligned", **{f"a{i}": b + 8})
    _refused(lib, fn, ok, INVALID, b"16-byte aligned", a11=b + 8, a12=200)


def test_im2col3_refusals(lib, buf):
    _, b = buf
    # x, col, batch, g, C, stream
    ok = [b, b, 2, 7, 64, None]
    fn = lib.vdr_op_im2col3
    for i in (0, 1):
        _refused(lib, fn, ok, INVALID, b"null argument", **{f"a{i}": None})
    for i in (2, 3):
        for v in (0, -1):
            _refused(lib, fn, ok, INVALID, b"bad shape", **{f"a{i}": v})
    _refused(lib, fn, ok, INVALID, b"2^31 rows", a2=1 << 20, a3=64)
    for Cc in (0, -8, 4, 60, 100):
        _refused(lib, fn, ok, UNSUPPORTED, b"C must be a positive multiple of 8", a4=Cc)
    for i in (0, 1):
        _refused(lib, fn, ok, INVALID, b"16-byte aligned", **{f"a{i}": b + 8})


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_sam_ops_without_a_gpu_fail_loudly(lib, buf):
    _, b = buf
    assert lib.vdr_op_layernorm_window(b, b, b, b, 2, 10, 4, 64, 1e-6, None) == NO_DEVICE
    assert b"no CPU path" in lib.vdr_last_error(None)
    assert lib.vdr_op_layernorm_mx_window(b, b, b, 1e-6, 2, 10, 4, 64, b, b, None) == NO_DEVICE
    for v in (0, 22, 25, 29):
        assert lib.vdr_op_linear_window(b, b, b, b, b, 2, 10, 4, 128, 64, v, None, 0, None) == NO_DEVICE
    assert lib.vdr_op_linear_window(b, b, None, b, b, 2, 10, 4, 128, 64, 26, b, 200, None) == NO_DEVICE
    assert lib.vdr_op_im2col3(b, b, 2, 7, 64, None) == NO_DEVICE
    assert b"no CPU path" in lib.vdr_last_error(None)


@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_window_index_is_the_oracles_partition_and_unpartition(batch, g, ws):
    from oracle import sam_oracle as so
    idx, valid = sr.window_index(batch, g, ws)
    rows = sr.window_rows(batch, g, ws)
    assert idx.shape == valid.shape == (rows,)
    # partition: entries encode (b, y, x), shifted by one so that the zero padding is told from token (0, 0, 0)
    b, y, x = torch.meshgrid(torch.arange(batch), torch.arange(g), torch.arange(g), indexing="ij")
    t = torch.stack([b + 1, y + 1, x + 1], dim=-1).float()
    win, pad_hw = so.window_partition(t, ws)
    win = win.reshape(-1, 3).long()
    assert win.shape[0] == rows
    assert torch.equal(valid, (win != 0).all(1)) and torch.equal(~valid, (win == 0).all(1))
    code = ((win[:, 0] - 1) * g + (win[:, 1] - 1)) * g + (win[:, 2] - 1)
    assert torch.equal(idx[valid], code[valid]) and bool((idx[~valid] == -1).all())
    assert int(valid.sum()) == batch * g * g and idx[valid].unique().numel() == batch * g * g
    # un-partition: windowed row numbers travel back to the token that idx names
    r = torch.arange(rows).float().reshape(-1, ws, ws, 1)
    back = so.window_unpartition(r, ws, pad_hw, (g, g)).reshape(-1).long()
    assert back.shape[0] == batch * g * g
    assert torch.equal(idx[back], torch.arange(batch * g * g))
    assert torch.equal(sr.token_to_window(batch, g, ws), back)


def test_designed_inputs_are_what_their_docstrings_say():
    for D in (64, 1280):
        x = sr.token_code_rows(8192, D)
        assert torch.equal(x, x.to(torch.bfloat16).float())
        assert torch.equal(x.mean(1), (torch.arange(8192) % 7 - 3).float())
        y = torch.nn.functional.layer_norm(x.double(), (D,), eps=1e-6)
        assert torch.equal(sr.decode_token_code(y, D), torch.arange(8192))
    # scale offsets: a bijection between (row, block) and the bytes of the array
    off = sr.mx_scale_offsets(300, torch.arange(512), 96)
    assert off.shape == (512, 3) and torch.equal(off.reshape(-1).sort().values, torch.arange(3 * 512))
    assert off[0, 0] == 0 and off[32, 0] == 1 and off[1, 0] == 2 and off[64, 1] == 512 + 64
    # im2col3 reference against a direct gather
    bits = torch.randint(-32768, 32768, (2 * 3 * 3, 8), dtype=torch.int16)
    col = sr.im2col3_ref(bits, 2, 3).reshape(2, 3, 3, 9, 8)
    img = bits.reshape(2, 3, 3, 8)
    for ky in range(3):
        for kx in range(3):
            for yy in range(3):
                for xx in range(3):
                    py, px = yy + ky - 1, xx + kx - 1
                    want = img[:, py, px] if 0 <= py < 3 and 0 <= px < 3 else torch.zeros(2, 8, dtype=torch.int16)
                    assert torch.equal(col[:, yy, xx, ky * 3 + kx], want)
