"""GPU: vdr_op_affinity_bits and vdr_op_bits_matvec (csrc/affinity.hip) at op level against the float64 restatement of their
definitions (tests/spectral_ref.py).

Designed inputs (nn_cosine_ref.designed: exactly 16 entries of +-1 per row, rn = 0.25, every score a multiple of 1/16, none at
0.2) must come back word for word, padding words 0: t in {1, 5, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300} (ragged words,
ragged tiles, more than one panel and tile), d in {32, 96, 448} (one short K step, a short last step, an odd number of steps
through the two staging buffers), P in {1, 3}, exclude_diag both ways, tau in {0.2, 0, 1/16} -- the last two a strict > on a
score that is attained.  Random inputs: symmetry bit for bit, and agreement with the float64 graph outside the band of the
entry-wise fp32 bound around tau, the band holding at most 1 % of the entries; one problem alone (its column tiles split into
runs) against the same problem among 300 (unsplit), word for word.  bits_matvec: integer-valued V (every order
exact) bit for bit, degree exact, random V within t u (B |V|), and independence of P bitwise."""
import numpy as np
import pytest
import torch

import nn_cosine_ref as nref
import spectral_ref as sref
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

TS = (1, 5, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300)
DIMS = (32, 96, 448)
PAIRS = 3
TAUS = (0.2, 0.0, 1.0 / 16.0)


_CACHE = {}


def _designed(t, d):
    """(x bf16 [3, t, d] on the CPU, float64 similarity) -- computed once per shape, shared, never written"""
    key = ("designed", t, d)
    if key not in _CACHE:
        x, _ = nref.designed(PAIRS, t, 1, d, seed=20000 * t + d)
        s = sref.similarity(x)
        assert not np.any(np.abs(s - 0.2) < 1e-3)  # multiples of 1/16: 0.1875 and 0.25 are the nearest
        _CACHE[key] = (x.to(torch.bfloat16), s)
    return _CACHE[key]


def _random(t, d):
    key = ("random", t, d)
    if key not in _CACHE:
        x = sref.random_maps(2, t, d, seed=11 + 1000 * t + d)  # (the seeds test_affinity_cpu.py checks the band share of)
        s = sref.similarity(x)
        _CACHE[key] = (x, s, sref.bound(x, s))
    return _CACHE[key]


def _want(s, tau, exclude_diag):
    b = s > float(np.float32(tau))
    if exclude_diag:
        i = np.arange(b.shape[1])
        b[:, i, i] = False
    return b


def _check_words(bits, want_bool, what):
    got = bits.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (want_bool.shape[0], want_bool.shape[1], sref.pitch(want_bool.shape[1])), what
    want = sref.pack(want_bool)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", TS)
def test_designed_inputs_are_exact(ops, t, d):
    x, s = _designed(t, d)
    xd = x.cuda()
    seen_attained = False
    for tau in TAUS:
        seen_attained |= bool(np.any(s == tau))
        for ex in (False, True):
            want = _want(s, tau, ex)
            b3 = ops.affinity_bits(xd, tau=tau, exclude_diag=ex)
            _check_words(b3, want, (t, d, tau, ex, 3))
            b1 = ops.affinity_bits(xd[:1], tau=tau, exclude_diag=ex)
            assert torch.equal(b1, b3[:1]), (t, d, tau, ex, "P = 1 against problem 0 of P = 3")
            assert torch.equal(ops.unpack_bits(b3, t).cpu(), torch.from_numpy(want))
    if t >= 31:
        assert seen_attained  # the strict > was tried on a score that is attained


def _raw_call(x, ldx, xs, t, P, d, tau, ex):
    """vdr_op_affinity_bits on caller-made buffers: bits with 4 guard words on either side, the work buffer exactly
    vdr_affinity_work_bytes inside a guarded allocation.  Returns bits after checking every guard."""
    from vdr import _lib
    lib = _lib.load()
    dev = x.device
    pitch = sref.pitch(t)
    wb = lib.vdr_affinity_work_bytes(P, t)
    work = torch.full((wb + 512,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((P * t * pitch + 8,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.vdr_op_affinity_bits(x.data_ptr(), ldx, xs, t, P, d, tau, int(ex), work.data_ptr() + 256, out.data_ptr() + 16, pitch,
                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.all(work[:256] == 0xA5) and torch.all(work[256 + wb:] == 0xA5)
    assert torch.all(out[:4] == -7) and torch.all(out[-4:] == -7)
    return out[4:-4].view(P, t, pitch)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", TS)
def test_strided_views_in_place_and_sentinels(ops, t, d):
    """The same data as columns [d, 2d) of a [P, 2 + t, 3d] buffer behind two prefix rows (ldx = 3d): the bits of the contiguous
    run; guards around bits and the work buffer untouched.  Problem stride 0: every problem is problem 0."""
    x, s = _designed(t, d)
    gen = torch.Generator().manual_seed(5)
    buf = torch.randint(-3, 4, (PAIRS, 2 + t, 3 * d), generator=gen).to(torch.bfloat16)
    buf[:, 2:, d:2 * d] = x
    buf = buf.cuda()
    view = buf[:, 2:, d:2 * d]
    for ex in (False, True):
        want = _want(s, 0.2, ex)
        got = _raw_call(view, 3 * d, (2 + t) * 3 * d, t, PAIRS, d, 0.2, ex)
        _check_words(got, want, (t, d, ex, "raw strided"))
        _check_words(ops.affinity_bits(view, tau=0.2, exclude_diag=ex), want, (t, d, ex, "ops strided"))
    got = _raw_call(view, 3 * d, 0, t, PAIRS, d, 0.2, False)
    _check_words(got, np.repeat(_want(s, 0.2, False)[:1], PAIRS, 0), (t, d, "stride 0"))
    got = ops.affinity_bits(x[:1].cuda().expand(PAIRS, t, d), tau=0.2)
    _check_words(got, np.repeat(_want(s, 0.2, False)[:1], PAIRS, 0), (t, d, "expand"))


@pytest.mark.parametrize("shape", ((300, 768), (257, 96)))
def test_graph_is_symmetric_bit_for_bit(ops, shape):
    t, d = shape
    x, _, _ = _random(t, d)
    for tau in (0.2, 0.0):
        b = ops.unpack_bits(ops.affinity_bits(x.cuda(), tau=tau), t)
        assert torch.equal(b, b.transpose(1, 2)), (shape, tau)


@pytest.mark.parametrize("shape", ((300, 768), (130, 13056)))
def test_random_inputs_match_outside_the_band(ops, shape):
    t, d = shape
    x, s, bnd = _random(t, d)
    tau = float(np.float32(0.2))
    got = ops.unpack_bits(ops.affinity_bits(x.cuda(), tau=0.2), t).cpu().numpy()
    clear = np.abs(s - tau) > bnd
    share = 1.0 - clear.mean()
    print(f"{shape}: share of entries inside the band {share:.3e}, set bits {got.mean():.3f}, max bound {bnd.max():.3e}")
    assert share <= 0.01, share
    assert 0.02 < got.mean() < 0.98  # a graph with both kinds of entries
    assert np.array_equal(got[clear], (s > tau)[clear]), int((got[clear] != (s > tau)[clear]).sum())
    assert got[:, np.arange(t), np.arange(t)].all()


def test_few_problems_take_the_split_path_and_many_the_unsplit_one(ops):
    """t = 130 is 2 panels x 2 column tiles.  One problem alone is 2 work items, so each panel's tiles are cut into 2 runs; 300
    problems are 600 items, above what the split aims for, so every panel walks both tiles in one run.  The split only decides
    which workgroup computes a word: the bits of the problem alone equal its bits as each of the 300, word for word."""
    t, d = 130, 96
    x, _, _ = _random(t, d)
    one = x[:1].cuda()
    alone = ops.affinity_bits(one, tau=0.2)
    share = float(ops.unpack_bits(alone, t).float().mean())
    assert 0.02 < share < 0.98, share  # a graph with both kinds of entries
    many = ops.affinity_bits(one.repeat(300, 1, 1), tau=0.2)
    assert many.shape == (300, t, sref.pitch(t))
    assert torch.equal(many, alone.expand_as(many)), torch.nonzero(many != alone)[:4].tolist()


MV_CASES = tuple((t, 32) for t in TS) + ((2100, 32), (300, 448))


def _mv_bits(ops, t, d):
    key = ("mvbits", t, d)
    if key not in _CACHE:
        if t == 2100:
            x, _ = nref.designed(PAIRS, t, 1, d, seed=77)
            x = x.to(torch.bfloat16)
        else:
            x = _designed(t, d)[0]
        _CACHE[key] = ops.affinity_bits(x.cuda(), tau=0.0)
    return _CACHE[key]


@pytest.mark.parametrize("nv", (1, 3, 8))
@pytest.mark.parametrize("case", MV_CASES)
def test_bits_matvec_is_exact_on_integers(ops, case, nv):
    t, d = case
    bits = _mv_bits(ops, t, d)
    B = ops.unpack_bits(bits, t)
    if t == 2100:
        assert sref.pitch(t) > 64 and B[0, 0, 64 * 32:].any()  # a lane walks more than one word, and finds bits there
    gen = torch.Generator().manual_seed(3 * t + nv)
    V = torch.randint(-64, 65, (PAIRS, t, nv), generator=gen).to(torch.float32).cuda()
    y, deg = ops.bits_matvec(bits, V, degree=True)
    want = torch.matmul(B.double(), V.double())  # integers below 2^24: exact in either precision
    assert y.dtype == torch.float32 and deg.dtype == torch.int32 and tuple(y.shape) == (PAIRS, t, nv)
    assert torch.equal(y.double(), want), (case, nv)
    assert torch.equal(deg.long(), B.sum(-1)), (case, nv)
    y1 = ops.bits_matvec(bits[1:2], V[1:2])
    assert torch.equal(y1, y[1:2])
    if nv == 1:
        assert torch.equal(ops.bits_matvec(bits, V[:, :, 0]), y[:, :, 0])


@pytest.mark.parametrize("case", ((300, 448), (2100, 32), (33, 32)))
def test_bits_matvec_random_values_and_problem_independence(ops, case):
    t, d = case
    bits = _mv_bits(ops, t, d)
    B = ops.unpack_bits(bits, t).double()
    gen = torch.Generator().manual_seed(t)
    V = torch.randn(PAIRS, t, 3, generator=gen).cuda()
    y = ops.bits_matvec(bits, V)
    want = torch.matmul(B, V.double())
    lim = t * sref.U * torch.matmul(B, V.double().abs())
    err = (y.double() - want).abs()
    print(f"{case}: max err / bound {(err / lim.clamp_min(1e-300)).max().item():.3e}")
    assert torch.all(err <= lim)
    for p in range(PAIRS):  # a problem's bits depend on neither P nor the position
        assert torch.equal(ops.bits_matvec(bits[p:p + 1], V[p:p + 1]), y[p:p + 1]), p
    rev = ops.bits_matvec(bits.flip(0), V.flip(0))
    assert torch.equal(rev.flip(0), y)
    assert torch.equal(ops.bits_matvec(bits, V), y)  # and from run to run


def test_refusals(ops):
    x = torch.zeros(1, 8, 48, dtype=torch.bfloat16).cuda()
    with pytest.raises(ValueError):
        ops.affinity_bits(x)
    with pytest.raises(ValueError):
        ops.affinity_bits(x[:, :, :32], tau=float("nan"))
    bits = ops.affinity_bits(x[:, :, :32])
    with pytest.raises(ValueError):
        ops.bits_matvec(bits, torch.zeros(1, 8, 9).cuda())
    with pytest.raises(ValueError):
        ops.bits_matvec(bits, torch.zeros(1, 7, 1).cuda())
    assert not ops.unpack_bits(bits, 8).any()  # zero rows: sim = 0 against everything, 0 > 0.2 is false
