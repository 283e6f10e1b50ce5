"""CPU: the float64 restatement of the affinity graph (tests/spectral_ref.py) against itself, an fp32 emulation in another
summation order against its bound, the band share of the random maps the GPU test uses, the bit packing (the reference's and
vdr.ops' plain-torch one), and the C ABI of the two ops: declarations, bindings, refusals before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nn_cosine_ref as nref
import spectral_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_graph_against_itself():
    x = sref.random_maps(2, 40, 64, seed=1)
    x[1, 7] = 0  # a zero row: sim = 0 against everything, itself included
    s = sref.similarity(x)
    assert np.array_equal(s, s.transpose(0, 2, 1))  # the product of the norms first: symmetric bit for bit, in float64 too
    diag = s[:, np.arange(40), np.arange(40)]
    assert np.allclose(np.delete(diag[1], 7), 1.0, atol=1e-12) and np.allclose(diag[0], 1.0, atol=1e-12) and diag[1, 7] == 0.0
    assert np.all(s[1, 7] == 0.0)
    # the definition differs from nn_cosine's only in the association
    assert np.allclose(s, nref.similarity(x, x), rtol=0, atol=1e-15)
    b, bx = sref.graph(x, 0.2), sref.graph(x, 0.2, exclude_diag=True)
    i = np.arange(40)
    assert b[0, i, i].all() and not bx[:, i, i].any() and not b[1, 7].any()
    off = ~np.eye(40, dtype=bool)
    assert np.array_equal(b[:, off], bx[:, off])
    # strict >: a score that is attained is not an edge
    xd, _ = nref.designed(1, 64, 1, 32, seed=3)
    sd = sref.similarity(xd)
    assert np.any(sd == 0.0625) and not sref.graph(xd, 0.0625)[sd == 0.0625].any() and sref.graph(xd, 0.0)[sd == 0.0625].all()


def _fp32_other_order(x: torch.Tensor) -> np.ndarray:
    """the definition in fp32 with numpy's pairwise sums: another summation order than the kernel's and than float64's"""
    xf = x.to(torch.float32).numpy()
    ss = (xf * xf).sum(-1, dtype=np.float32)
    rn = (np.float32(1.0) / np.maximum(np.sqrt(ss, dtype=np.float32), np.float32(1e-8))).astype(np.float32)
    dot = np.stack([(xf[p][:, None, :] * xf[p][None, :, :]).sum(-1, dtype=np.float32) for p in range(xf.shape[0])])
    out = dot * (rn[:, :, None] * rn[:, None, :])
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("shape", ((60, 32), (60, 96), (60, 448), (24, 13056)))
def test_fp32_emulation_stays_below_the_bound(shape):
    t, d = shape
    x = sref.random_maps(2, t, d, seed=5 + d)
    s = sref.similarity(x)
    b = sref.bound(x, s)
    e = _fp32_other_order(x)
    assert np.array_equal(e, e.transpose(0, 2, 1))  # symmetric bit for bit in fp32 as well
    ratio = (np.abs(e.astype(np.float64) - s) / b).max()
    print(f"{shape}: max |fp32 - f64| / bound = {ratio:.4f}, max bound {b.max():.3e}")
    assert ratio < 1.0


@pytest.mark.parametrize("shape", ((300, 768), (130, 13056), (257, 96)))
def test_band_share_of_the_gpu_tests_random_maps(shape):
    """tests/test_affinity_gpu.py caps the share of entries it cannot judge at 1 %: the reference alone stays under that"""
    t, d = shape
    x = sref.random_maps(2, t, d, seed=11 + 1000 * t + d)
    s = sref.similarity(x)
    share = sref.band_share(s, sref.bound(x, s), 0.2)
    edges = (s > 0.2).mean()
    print(f"{shape}: band share {share:.3e}, edge share {edges:.3f}")
    assert share <= 0.01 and 0.02 < edges < 0.98


@pytest.mark.parametrize("t", (1, 31, 32, 33, 64, 65, 129))
def test_pack_unpack_round_trip(t):
    from vdr import ops
    rng = np.random.default_rng(t)
    b = rng.random((2, t, t)) < 0.5
    b[0, :, t - 1] = True  # the last column, bit (t - 1) & 31 of the last used word
    b[1, :, 0] = True
    w = sref.pack(b)
    assert w.dtype == np.int32 and w.shape == (2, t, sref.pitch(t)) and sref.pitch(t) % 4 == 0 and sref.pitch(t) * 32 >= t
    assert sref.pitch(t) == ops.bits_pitch(t) == -(-(-(-t // 32)) // 4) * 4
    assert np.array_equal(sref.unpack(w, t), b)
    for i, j in ((0, 0), (0, t - 1), (t - 1, t // 2)):
        assert bool((int(w[0, i, j >> 5]) >> (j & 31)) & 1) == bool(b[0, i, j])
    tw = ops.pack_bits(torch.from_numpy(b))
    assert tw.dtype == torch.int32 and np.array_equal(tw.numpy(), w)
    assert np.array_equal(ops.unpack_bits(torch.from_numpy(w), t).numpy(), b)
    with pytest.raises(ValueError):
        ops.unpack_bits(torch.from_numpy(w), t + 1)


def test_abi_declarations_and_bindings():
    from vdr import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdr.h")).read(), flags=re.S)
    for name, nargs in (("vdr_affinity_work_bytes", 2), ("vdr_op_affinity_bits", 12), ("vdr_op_bits_matvec", 9)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    lib = _lib.load()
    assert lib.vdr_affinity_work_bytes(3, 130) == 3 * 256 * 4 and lib.vdr_affinity_work_bytes(1, 128) == 512
    assert lib.vdr_affinity_work_bytes(0, 5) == 0 and lib.vdr_affinity_work_bytes(2, 0) == 0


def test_ops_refuse_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    buf = (C.c_char * 256)()
    b = (C.addressof(buf) + 15) & ~15
    ok = [b, 32, 32 * 8, 8, 1, 32, 0.2, 0, b, b, 4, None]  # x, ldx, x_stride, t, pairs, d, tau, exclude_diag, work, bits, pitch, stream

    def aff(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.vdr_op_affinity_bits(*a)
    for i in (0, 8, 9):
        assert aff(**{f"a{i}": None}) == -1, i  # VDR_ERR_INVALID
    assert b"null" in lib.vdr_last_error(None)
    assert aff(a5=48) == -7 and b"multiple of 32" in lib.vdr_last_error(None)  # VDR_ERR_UNSUPPORTED
    for kw in (dict(a3=0), dict(a4=0), dict(a5=0), dict(a1=16), dict(a2=-8), dict(a1=36), dict(a2=4), dict(a0=b + 2), dict(a9=b + 4),
               dict(a10=1), dict(a10=8), dict(a3=129), dict(a6=float("nan")), dict(a4=2 ** 30, a3=8)):
        assert aff(**kw) == -1, kw
    okm = [b, 4, 8, 1, b, 1, b, None, None]  # bits, pitch, t, pairs, v, nv, y, degree, stream

    def mv(**kw):
        a = list(okm)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.vdr_op_bits_matvec(*a)
    for i in (0, 4, 6):
        assert mv(**{f"a{i}": None}) == -1, i
    for nv in (0, 9, -1):
        assert mv(a5=nv) == -7, nv
    for kw in (dict(a1=8), dict(a2=0), dict(a3=0), dict(a0=b + 4), dict(a4=b + 2), dict(a7=b + 1), dict(a3=2 ** 30)):
        assert mv(**kw) == -1, kw
    if not torch.cuda.is_available():
        assert aff() == -2 and mv() == -2  # VDR_ERR_NO_DEVICE: no CPU path behind the boundary
