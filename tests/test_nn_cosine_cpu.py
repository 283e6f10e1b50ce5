"""CPU: cosine nearest neighbours and correspondences -- vdr_op_nn_cosine / vdr_nn_cosine_work_bytes are declared, bound and
exported and refuse bad arguments before they touch a device; the float64 restatement (tests/nn_cosine_ref.py) is torch's
cosine_similarity + max; an fp32 evaluation in another summation order stays inside the restatement's bound; best_buddies
on a hand-written case; find_correspondences' host-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nn_cosine_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")


def test_header_binding_and_exports_declare_the_nn_cosine_entry_points():
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"size_t vdr_nn_cosine_work_bytes\(int pairs, int tx, int ty\);", src)
    assert re.search(r"int vdr_op_nn_cosine\(const void\* x, int64_t ldx, int64_t x_stride, int tx,\s*"
                     r"const void\* y, int64_t ldy, int64_t y_stride, int ty,\s*int pairs, int d, void\* work,\s*"
                     r"float\* row_sim, int32_t\* row_idx, float\* col_sim, int32_t\* col_idx, void\* stream\);", src)
    assert re.search(r"#define VDR_ABI_VERSION 8\b", src)
    # header and binding declare the same set of symbols
    declared = set(re.findall(r"\b(vdr_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert {"vdr_op_nn_cosine", "vdr_nn_cosine_work_bytes"} <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_nn_cosine") and hasattr(lib, "vdr_nn_cosine_work_bytes")
    assert lib.vdr_abi_version() == 8
    import vdr
    from vdr import ops
    assert callable(ops.nn_cosine) and callable(ops.best_buddies) and callable(vdr.VitDescriptorModel.find_correspondences)
    assert [f for f in vdr.Correspondences.__dataclass_fields__][:8] == ["nn12", "sim12", "nn21", "sim21", "saliency1", "saliency2",
                                                                        "mask", "grid"]


def test_op_nn_cosine_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    x, y, work, rs, ri, cs, ci = (base + 1024 * k for k in range(7))

    def call(x=x, ldx=32, xs=96, tx=3, y=y, ldy=32, ys=64, ty=2, pairs=2, d=32, work=work, rs=rs, ri=ri, cs=cs, ci=ci):
        return lib.vdr_op_nn_cosine(x, ldx, xs, tx, y, ldy, ys, ty, pairs, d, work, rs, ri, cs, ci, None)

    for kw in (dict(d=16, ldx=16, ldy=16), dict(d=48, ldx=48, ldy=48), dict(d=8), dict(d=33, ldx=40, ldy=40)):
        assert call(**kw) == -7, kw  # VDR_ERR_UNSUPPORTED
        assert b"d" in lib.vdr_last_error(None)
    invalid = [dict(x=None), dict(y=None), dict(work=None), dict(rs=None), dict(ri=None), dict(cs=None), dict(ci=None),
               dict(pairs=0), dict(pairs=-1), dict(tx=0), dict(ty=-2), dict(d=0), dict(d=-32),
               dict(ldx=24), dict(ldy=31), dict(d=64), dict(xs=-96), dict(ys=-8),
               dict(x=x + 2), dict(x=x + 8), dict(y=y + 4), dict(work=work + 8), dict(rs=rs + 4), dict(ri=ri + 8), dict(cs=cs + 4),
               dict(ci=ci + 12), dict(ldx=36), dict(ldy=44), dict(xs=100), dict(ys=68),
               dict(pairs=2, tx=2 ** 30), dict(pairs=3, ty=2 ** 30), dict(pairs=2 ** 16, tx=2 ** 15)]
    for kw in invalid:
        assert call(**kw) == -1, kw  # VDR_ERR_INVALID
    # a stride of 0 and a null column side are well formed: such a call gets as far as the device check or the launch
    assert call(xs=0, cs=None, ci=None) in (0, -2, -3)


def test_work_bytes_is_monotone_and_positive():
    from vdr import _lib
    lib = _lib.load()
    wb = lib.vdr_nn_cosine_work_bytes
    sizes = (1, 2, 5, 127, 128, 129, 196, 729, 3969, 20000)
    for pairs in (1, 2, 3, 8, 64, 1000):
        for tx in sizes:
            for ty in sizes:
                w = wb(pairs, tx, ty)
                assert w > 0 and w % 16 == 0
                # at least the row norms and one (value, index) per output
                assert w >= 4 * pairs * (tx + ty) + 8 * pairs * (tx + ty)
                assert wb(pairs + 1, tx, ty) >= w and wb(pairs, tx + 1, ty) >= w and wb(pairs, tx, ty + 1) >= w
                assert wb(2 * pairs, tx, ty) > w and wb(pairs, tx + 128, ty) > w and wb(pairs, tx, ty + 128) > w
    assert wb(0, 5, 5) == 0 and wb(1, 0, 5) == 0 and wb(1, 5, -1) == 0


@pytest.mark.parametrize("shape", ((1, 1, 32), (5, 3, 96), (130, 257, 64)))
def test_the_restatement_is_cosine_similarity_plus_max(shape):
    tx, ty, d = shape
    gen = torch.Generator().manual_seed(tx + ty + d)
    x = torch.randn(2, tx, d, generator=gen).to(torch.bfloat16)
    y = torch.randn(2, ty, d, generator=gen).to(torch.bfloat16)
    s = nref.similarity(x, y)
    want = torch.nn.functional.cosine_similarity(x.double()[:, :, None, :], y.double()[:, None, :, :], dim=-1)
    assert np.abs(s - want.numpy()).max() <= 1e-12
    rs, ri, cs, ci = nref.nearest(s)
    assert np.abs(rs - want.max(2).values.numpy()).max() <= 1e-12 and np.abs(cs - want.max(1).values.numpy()).max() <= 1e-12
    assert np.array_equal(np.take_along_axis(s, ri[:, :, None].astype(np.int64), 2)[:, :, 0], s.max(2))
    assert np.array_equal(np.take_along_axis(s, ci[:, None, :].astype(np.int64), 1)[:, 0, :], s.max(1))
    # a zero row has sim = 0 against everything
    x[0, 0] = 0
    assert np.all(nref.similarity(x, y)[0, 0] == 0.0)


def test_designed_inputs_are_exact_in_any_precision_and_have_ties():
    x, y = nref.designed(2, 130, 257, 64, seed=1)
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.all((x != 0).sum(-1) == 16) and torch.all((y != 0).sum(-1) == 16)
    s = nref.similarity(x, y)
    assert np.array_equal(s * 16, np.round(s * 16)) and np.abs(s).max() <= 1.0
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    assert nref.rows_with_ties(s) > 1 and nref.rows_with_ties(s.transpose(0, 2, 1)) > 1
    # the planted duplicates resolve to the lowest index
    _, ri, _, ci = nref.nearest(s)
    assert ri[0, 1] == 0 and ri[0, 70] == 40 and ci[0, 1] == 0 and ci[0, 64] == 11
    # asymmetric: the transposed problem has another answer
    assert not np.array_equal(nref.similarity(y[:, :130], x)[:, :, :130], s[:, :, :130])


@pytest.mark.parametrize("d", (32, 96, 448, 13056))
def test_an_fp32_evaluation_in_another_order_stays_inside_the_bound(d):
    tx, ty = (33, 47) if d < 1000 else (9, 12)
    gen = torch.Generator().manual_seed(d)
    x = torch.randn(1, tx, d, generator=gen).to(torch.bfloat16)
    y = torch.randn(1, ty, d, generator=gen).to(torch.bfloat16)
    s = nref.similarity(x, y)
    b = nref.bound(x, y, s)
    xf, yf = x.float().numpy(), y.float().numpy()
    # fp32 throughout: sequential sums from the LAST channel to the first (no pairwise tree, no wider accumulator)
    dot = np.zeros((tx, ty), np.float32)
    ssx, ssy = np.zeros(tx, np.float32), np.zeros(ty, np.float32)
    for c in range(d - 1, -1, -1):
        dot += np.outer(xf[0, :, c], yf[0, :, c])
        ssx += xf[0, :, c] * xf[0, :, c]
        ssy += yf[0, :, c] * yf[0, :, c]
    one, eps = np.float32(1.0), np.float32(1e-8)
    got = (dot * (one / np.maximum(np.sqrt(ssx), eps))[:, None]) * (one / np.maximum(np.sqrt(ssy), eps))[None, :]
    assert got.dtype == np.float32
    ratio = np.abs(got.astype(np.float64) - s[0]) / b[0]
    print(f"d={d}: max err / bound {ratio.max():.4f}, max bound {b.max():.3e}")
    assert ratio.max() <= 1.0


def test_best_buddies_on_a_hand_written_case():
    from vdr import ops
    # 4 rows of x, 3 rows of y.  x0 -> y1 -> x0 (mutual); x1 -> y1 -> x0 (not mutual); x2 -> y2 -> x2 (mutual);
    # x3 -> y0 -> x1 (not mutual)
    row_idx = torch.tensor([[1, 1, 2, 0]], dtype=torch.int32)
    col_idx = torch.tensor([[1, 0, 2]], dtype=torch.int32)
    got = ops.best_buddies(row_idx, col_idx)
    assert got.dtype == torch.bool and got.shape == (1, 4)
    assert got.tolist() == [[True, False, True, False]]
    two = ops.best_buddies(torch.cat([row_idx, torch.tensor([[0, 0, 0, 0]], dtype=torch.int32)]),
                           torch.cat([col_idx, torch.tensor([[3, 0, 0]], dtype=torch.int32)]))
    assert two.tolist() == [[True, False, True, False], [False, False, False, True]]
    with pytest.raises(ValueError, match="best_buddies"):
        ops.best_buddies(row_idx[0], col_idx)


def test_nn_cosine_refuses_on_the_host_before_the_library_is_called():
    from vdr import ops
    x = torch.zeros(2, 4, 32, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="HIP device"):
        ops.nn_cosine(x, x)
    with pytest.raises(TypeError, match=r"\[P, t, d\]"):
        ops.nn_cosine(x[0], x)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.nn_cosine(x.half(), x)


def test_find_correspondences_refusals_need_no_device():
    import vdr
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg = vdr.ARCHS["vit_tiny16_224"]
    m.model_name = "vit_tiny16_224"
    a, b = torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 48)
    with pytest.raises(ValueError, match="same shape"):
        m.find_correspondences(a, b)
    with pytest.raises(ValueError, match="same shape"):
        m.find_correspondences(a, torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="facet"):
        m.find_correspondences(a, a, facet="keys")
    with pytest.raises(ValueError, match="hierarchy"):
        m.find_correspondences(a, a, hierarchy=4)
    with pytest.raises(ValueError, match="out of range"):
        m.find_correspondences(a, a, layer=12)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.find_correspondences(a, a)
    m.cfg = vdr.ARCHS["dinov2"]  # patch embedding only: no blocks
    with pytest.raises(ValueError, match="no blocks"):
        m.find_correspondences(a, a, facet="token")
    m.cfg = vdr.VdrConfig(0, 0, 3, 64, 2, 2, 256)  # token model
    with pytest.raises(ValueError, match="token model"):
        m.find_correspondences(a, a)
    m.cfg = vdr.VdrConfig(32, 8, 3, 64, 2, 2, 256, pre_ln=False)
    with pytest.raises(ValueError, match="pre-LN"):
        m.find_correspondences(a, a)
    m.cfg = vdr.ARCHS["siglip_base16_224"]
    with pytest.raises(ValueError, match="CLS"):
        m.find_correspondences(a, a)
