"""GPU: vdr_op_mahalanobis (csrc/mahalanobis.hip) at op level against the float64 restatement of its definition
(tests/mahalanobis_ref.py).

Designed inputs, bit for bit (`_designed`): x and mean small integers with |x - mean| <= 4; whitening rows with at most 8
non-zeros from {+-1, +-1/2, +-1/4}.  Two kinds of entries need the lo operands:
  * whitening entries +-(1 + 2^-10) (w_hi = 1, w_lo = 2^-10) in the channels c % 16 == 5, met by the rows i % 7 == 3;
  * means m + 2^-7 in the channels c % 16 == 11, where the rows i % 7 == 5 hold integers 2 .. 4 away, so that x - mean needs 9 or
    10 significant bits (z_lo = -+2^-7); every other row holds the mean itself there (m + 2^-7 is a bf16 value) and z = 0.
Every y has at most 12 significant bits, so its square is exact in fp32, and per row the squares are multiples of one power of
two whose sum stays below 2^24 of them: any order of the sums is exact.  `_designed` asserts all of that in integers, and that
dropping either lo operand changes the special rows.
R in {1, 127, 128, 129, 300} (ragged panels, more than one), k in {1, 128, 129, 260} (ragged tiles, more than one), d in
{32, 96, 448} (half a 64-column step, one and a half, seven), problems in {1, 3}, and a [problems, imgs, t, d] operand."""
import numpy as np
import pytest
import torch

import mahalanobis_ref as mr
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

RS = (1, 127, 128, 129, 300)
KS = (1, 128, 129, 260)
DS = (32, 96, 448)


_CACHE = {}


def _sig_bits_ok(v, bits):
    m, _ = np.frexp(v)
    return bool((np.ldexp(m, bits) == np.round(np.ldexp(m, bits))).all())


def _designed(R, k, d, seed=0):
    """one problem: (x [R, d] fp32 holding bf16 values, mean [d] fp32, w [k, d] fp32, d2 [R] float64) -- computed once per
    case, shared, never written"""
    key = (R, k, d, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(1000 * R + 10 * k + d + 7919 * seed)
    ch = np.arange(d)
    ca, cb = ch % 16 == 5, ch % 16 == 11
    reg = ~(ca | cb)
    mean = rng.integers(-2, 3, d).astype(np.float64)
    mean[cb] = rng.integers(-1, 2, cb.sum()) + 2.0 ** -7
    rows = np.arange(R)
    ra, rb = rows % 7 == 3, rows % 7 == 5
    x = np.tile(mean, (R, 1))
    delta = rng.integers(-2, 3, (R, d)).astype(np.float64)
    plain = ~(ra | rb)
    x[np.ix_(plain, reg)] += delta[np.ix_(plain, reg)]
    x[np.ix_(ra, ca)] += rng.choice([-1.0, 1.0], (int(ra.sum()), int(ca.sum())))
    x[np.ix_(rb, cb)] += rng.choice([-3.0, -2.0, 3.0], (int(rb.sum()), int(cb.sum()))) + (-2.0 ** -7)  # integers 2 .. 4 away
    assert (np.abs(x - mean[None, :]) <= 4.0).all() and (np.abs(x) <= 5.0).all()
    w = np.zeros((k, d))
    regc = np.flatnonzero(reg)
    for j in range(k):
        nnz = int(rng.integers(0, 7))
        cols = rng.choice(regc, nnz, replace=False)
        w[j, cols] = rng.choice([1.0, 0.5, 0.25], nnz) * rng.choice([-1.0, 1.0], nnz)
    special = sorted({0, k - 1, k // 2, min(127, k - 1), min(128, k - 1)})  # first, last, either side of the tile boundary
    for n, j in enumerate(special):
        w[j, np.flatnonzero(ca)[n % int(ca.sum())]] = (1.0 + 2.0 ** -10) * (-1.0) ** n
        w[j, np.flatnonzero(cb)[n % int(cb.sum())]] = (0.5, 0.25)[n % 2] * (-1.0) ** (n // 2)
    assert ((w != 0).sum(-1) <= 8).all()
    x32, mean32, w32 = x.astype(np.float32), mean.astype(np.float32), w.astype(np.float32)
    assert (x32 == x).all() and (mr.bf16_rn(x32) == x).all() and (mean32 == mean).all() and (w32 == w).all()
    y = mr.y(x32, mean32, w32)
    ref = (y * y).sum(-1)
    # the design's conditions, in integers: every y has <= 12 significant bits; per row the squares are multiples of one power
    # of two and sum to less than 2^24 of it; the products of a y are multiples of 2^-12 below 2^12 in all
    assert _sig_bits_ok(y, 12)
    T = np.round(y * y * 2.0 ** 24).astype(np.int64)  # (every y is a multiple of 2^-12 below 2^4)
    assert (T == y * y * 2.0 ** 24).all()
    for i in range(R):
        low = int(np.bitwise_or.reduce(T[i]))
        if low:
            assert int(T[i].sum()) // (low & -low) < 2 ** 24, i
    zc = mr.centre(x32, mean32)
    assert (np.abs(zc) @ np.abs(w).T * 2.0 ** 12).max() < 2 ** 24
    if R > 5:  # both kinds of special rows exist: without z_lo or without w_lo their distances differ
        zh, zl = mr.split(zc)
        wh, wl = mr.split(w32)
        assert (zl[rb] != 0).any() and (wl != 0).any()
        no_wlo = ((zh @ wh.T + zl @ wh.T) ** 2).sum(-1)
        no_zlo = ((zh @ wh.T + zh @ wl.T) ** 2).sum(-1)
        assert (no_wlo[ra] != ref[ra]).all() and (no_zlo[rb] != ref[rb]).all()
    _CACHE[key] = (x32, mean32, w32, ref)
    return _CACHE[key]


def _stack(R, k, d, problems):
    parts = [_designed(R, k, d, s) for s in range(problems)]
    return tuple(np.stack([p[n] for p in parts]) for n in range(4))


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def _same_bits(got: torch.Tensor, ref64: np.ndarray):
    ref32 = ref64.astype(np.float32)
    assert (ref32.astype(np.float64) == ref64).all()  # (the design: the float64 result is an fp32 value)
    return np.array_equal(got.cpu().numpy().view(np.uint32), ref32.view(np.uint32))


@pytest.mark.parametrize("problems", (1, 3))
@pytest.mark.parametrize("d", DS)
def test_designed_inputs_bit_for_bit(ops, d, problems):
    for R in RS:
        for k in KS:
            x, mean, w, ref = _stack(R, k, d, problems)
            got = ops.mahalanobis(_gpu(x, torch.bfloat16), _gpu(mean), _gpu(w))
            assert tuple(got.shape) == (problems, R) and got.dtype == torch.float32
            assert _same_bits(got, ref), (R, k, d)


def test_fp32_rows_are_rounded_once(ops):
    x, mean, w, ref = _stack(129, 129, 96, 2)
    # a perturbation below half a bf16 ulp of every |x| >= 1: the one rounding to bf16 removes it
    x32 = np.where(np.abs(x) >= 1.0, x * np.float32(1.0 + 2.0 ** -11), x).astype(np.float32)
    assert (x32 != x).any() and (mr.bf16_rn(x32) == x).all()
    assert _same_bits(ops.mahalanobis(_gpu(x32), _gpu(mean), _gpu(w)), ref)


def test_images_of_a_problem_and_joint(ops):
    x, mean, w, ref = _stack(129, 129, 96, 2)
    xg = _gpu(x, torch.bfloat16)
    four = xg.reshape(2, 3, 43, 96)  # [problems, imgs, t, d]
    assert _same_bits(ops.mahalanobis(four, _gpu(mean), _gpu(w)), ref)
    # images a gap apart
    buf = torch.full((2, 3, 50, 96), float("nan"), dtype=torch.bfloat16).cuda()
    buf[:, :, 4:47] = four
    view = buf[:, :, 4:47]
    assert ops.kmeans_operand(view).x.data_ptr() == view.data_ptr()  # (read in place)
    assert _same_bits(ops.mahalanobis(view, _gpu(mean), _gpu(w)), ref)
    # joint: the rows of all images of a [P, t, d] operand as one problem
    got = ops.mahalanobis(xg[0].reshape(3, 43, 96), _gpu(mean[:1]), _gpu(w[:1]), joint=True)
    assert tuple(got.shape) == (1, 129) and _same_bits(got, ref[:1])


def test_views_are_read_in_place(ops):
    R, k, d = 129, 129, 96
    x, mean, w, ref = _stack(R, k, d, 3)
    xg, mg, wg = _gpu(x, torch.bfloat16), _gpu(mean), _gpu(w)
    nan = float("nan")
    wide = torch.full((3, R, 3 * d), nan, dtype=torch.bfloat16).cuda()  # a column slice of a 3 d wide buffer
    wide[:, :, d:2 * d] = xg
    tall = torch.full((3, R + 12, d), nan, dtype=torch.bfloat16).cuda()  # rows behind a prefix, NaN rows before and after
    tall[:, 5:5 + R] = xg
    for view in (wide[:, :, d:2 * d], tall[:, 5:5 + R]):
        assert ops.kmeans_operand(view).x.data_ptr() == view.data_ptr()
        assert _same_bits(ops.mahalanobis(view, mg, wg), ref)
    # whitening rows with NaN rows behind them, means inside a wider buffer
    wbuf = torch.full((3, k + 3, d), nan, dtype=torch.float32).cuda()
    wbuf[:, :k] = wg
    mbuf = torch.full((3, 2 * d), nan, dtype=torch.float32).cuda()
    mbuf[:, :d] = mg
    wv, mv = wbuf[:, :k], mbuf[:, :d]
    assert ops._mahalanobis_model(wv, "whiten", (k, d), 3, wv.device)[0].data_ptr() == wv.data_ptr()
    assert _same_bits(ops.mahalanobis(tall[:, 5:5 + R], mv, wv), ref)
    # a NaN row poisons its own distance and no other
    bad = xg.clone()
    bad[1, 77, 3] = nan
    got = ops.mahalanobis(bad, mg, wg)
    assert bool(torch.isnan(got[1, 77])) and int(torch.isnan(got).sum()) == 1
    got[1, 77] = float(ref[1, 77])
    assert _same_bits(got, ref)


def test_problem_stride_zero_on_either_side(ops):
    R, k, d = 129, 129, 96
    x, mean, w, ref = _stack(R, k, d, 3)
    xg, mg, wg = _gpu(x, torch.bfloat16), _gpu(mean), _gpu(w)
    # one map under three models: the bits of the map copied three times
    shared = xg[0].unsqueeze(0).unsqueeze(0).expand(3, 1, R, d)
    assert ops.kmeans_operand(shared).problem_stride == 0
    got = ops.mahalanobis(shared, mg, wg)
    assert _same_bits(got[:1], ref[:1]) and torch.equal(got, ops.mahalanobis(shared.contiguous(), mg, wg))
    assert not torch.equal(got[1], got[0])
    # one model under three maps: the bits of the model copied three times
    me, we = mg[:1].expand(3, d), wg[:1].expand(3, k, d)
    assert ops._mahalanobis_model(we, "whiten", (k, d), 3, we.device)[1] == 0  # (taken as it is)
    got = ops.mahalanobis(xg, me, we)
    assert _same_bits(got[:1], ref[:1]) and torch.equal(got, ops.mahalanobis(xg, me.contiguous(), we.contiguous()))
    # both: one map under one model, three times
    assert torch.equal(ops.mahalanobis(shared, me, we), got[:1].expand(3, R))


def test_output_inside_a_guarded_buffer(ops):
    R, k, d = 129, 260, 32
    x, mean, w, ref = _stack(R, k, d, 3)
    guard = 12345.5
    big = torch.full((3 * R + 64,), guard, dtype=torch.float32).cuda()
    out = big[3:3 + 3 * R].view(3, R)  # 4-byte aligned only
    assert out.data_ptr() % 16 == 12
    got = ops.mahalanobis(_gpu(x, torch.bfloat16), _gpu(mean), _gpu(w), out=out)
    assert got.data_ptr() == out.data_ptr() and _same_bits(got, ref)
    assert bool((big[:3] == guard).all()) and bool((big[3 + 3 * R:] == guard).all())


def _random(R, k, d, seed):
    rng = np.random.default_rng(seed)
    x = mr.bf16_rn(rng.normal(size=(R, d)) + 0.5).astype(np.float32)
    mean = x.mean(0).astype(np.float32)
    w = (rng.normal(size=(k, d)) * np.logspace(0, 1.5, k)[:, None] / np.sqrt(d)).astype(np.float32)
    return x, mean, w


def test_bits_do_not_depend_on_the_batch(ops):
    R, k, d = 300, 260, 96
    parts = [_random(R, k, d, s) for s in (1, 2, 3)]
    xg = _gpu(np.stack([p[0] for p in parts]), torch.bfloat16)
    mg, wg = _gpu(np.stack([p[1] for p in parts])), _gpu(np.stack([p[2] for p in parts]))
    batch = ops.mahalanobis(xg, mg, wg)
    for p in range(3):
        alone = ops.mahalanobis(xg[p:p + 1], mg[p:p + 1], wg[p:p + 1])
        assert torch.equal(alone[0], batch[p])
    order = [2, 0, 1]
    moved = ops.mahalanobis(xg[order], mg[order], wg[order])
    assert torch.equal(moved, batch[order])
    assert torch.equal(ops.mahalanobis(xg, mg, wg), batch)  # run to run
    # and not on R: the first rows alone
    assert torch.equal(ops.mahalanobis(xg[:, :77], mg, wg), batch[:, :77])


@pytest.mark.parametrize("shape", ((300, 768, 768), (130, 64, 416)))
def test_random_maps_stay_inside_the_bound(ops, shape):
    R, k, d = shape
    x, mean, w = _random(R, k, d, R + k)
    ref, bound = mr.d2(x, mean, w), mr.d2_bound(x, mean, w)
    got = ops.mahalanobis(_gpu(x, torch.bfloat16).unsqueeze(0), _gpu(mean).unsqueeze(0), _gpu(w).unsqueeze(0))[0].cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print(f"R = {R}, k = {k}, d = {d}: worst |gpu - float64| / bound {ratio.max():.4f}, worst relative {np.max(np.abs(got - ref) / ref):.3e}")
    assert (ratio <= 1.0).all()  # every row, no cap
    # against fp32 torch on the fp32 operands: what the definition leaves out (the split residuals) is below 1e-4
    xt = torch.from_numpy(x).cuda()
    full = ((xt.double() - _gpu(mean).double()) @ _gpu(w).double().T).square().sum(-1).cpu().numpy()
    assert (np.abs(got - full) <= 1e-4 * full).all()


def test_python_refusals(ops):
    x = torch.zeros((2, 8, 64), dtype=torch.bfloat16).cuda()
    mean, w = torch.zeros((2, 64)).cuda(), torch.zeros((2, 3, 64)).cuda()
    assert tuple(ops.mahalanobis(x, mean, w).shape) == (2, 8)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mahalanobis(torch.zeros((2, 8, 48), dtype=torch.bfloat16).cuda(), mean[:, :48], w[:, :, :48])
    with pytest.raises(TypeError):
        ops.mahalanobis(x.half(), mean, w)
    with pytest.raises(TypeError, match="HIP device"):
        ops.mahalanobis(x.cpu(), mean, w)
    with pytest.raises(ValueError, match="joint"):
        ops.mahalanobis(x.unsqueeze(0), mean[:1], w[:1], joint=True)
    with pytest.raises(ValueError, match="empty"):
        ops.mahalanobis(x[:, :0], mean, w)
    for bad in (mean[:1], mean[:, :32], mean.double(), mean.cpu(), None):
        with pytest.raises(ValueError, match="mean"):
            ops.mahalanobis(x, bad, w)
    for bad in (w[:1], w[:, :, :32], w.double(), w.cpu(), w[0], None):
        with pytest.raises(ValueError, match="whiten"):
            ops.mahalanobis(x, mean, bad)
    with pytest.raises(ValueError, match="1..2048"):
        ops.mahalanobis(x, mean, torch.zeros((2, 2049, 64)).cuda())
    with pytest.raises(ValueError, match="1..2048"):
        ops.mahalanobis(x, mean, w[:, :0])
    for bad in (torch.zeros((2, 9)).cuda(), torch.zeros((2, 8), dtype=torch.float64).cuda(), torch.zeros((2, 8)), torch.zeros((2, 16)).cuda()[:, ::2]):
        with pytest.raises(ValueError, match="out"):
            ops.mahalanobis(x, mean, w, out=bad)
    assert tuple(ops.mahalanobis(x, mean, torch.zeros((2, 2048, 64)).cuda()).shape) == (2, 8)  # (the largest k)


def test_c_level_refusals_on_the_device(ops):
    from vdr import _lib
    lib = _lib.load()
    x = torch.zeros((2, 8, 64), dtype=torch.bfloat16).cuda()
    mean, w, out = torch.zeros((2, 64)).cuda(), torch.zeros((2, 3, 64)).cuda(), torch.full((2, 8), 7.0).cuda()

    def call(**kw):
        a = dict(x=x.data_ptr(), ld=64, image_stride=0, problem_stride=512, problems=2, imgs=1, t=8, d=64, mean=mean.data_ptr(),
                 mean_stride=64, whiten=w.data_ptr(), whiten_stride=192, k=3, d2=out.data_ptr(), stream=None)
        a.update(kw)
        return lib.vdr_op_mahalanobis(*a.values())

    INVALID, UNSUPPORTED = -1, -7
    for name in ("x", "mean", "whiten", "d2"):
        assert call(**{name: None}) == INVALID and b"null" in lib.vdr_last_error(None)
    assert call(d=48) == UNSUPPORTED and b"multiple of 32" in lib.vdr_last_error(None)
    for k in (0, 2049):
        assert call(k=k, whiten_stride=0) == UNSUPPORTED and b"1..2048" in lib.vdr_last_error(None)
    for kw in (dict(x=x.data_ptr() + 2), dict(mean=mean.data_ptr() + 4), dict(whiten=w.data_ptr() + 8), dict(d2=out.data_ptr() + 2),
               dict(ld=68), dict(problem_stride=516), dict(image_stride=4), dict(mean_stride=65), dict(whiten_stride=193)):
        assert call(**kw) == INVALID and b"aligned" in lib.vdr_last_error(None), kw
    assert call(problems=2 ** 20, imgs=2 ** 6, t=2 ** 5) == INVALID and b"2^31" in lib.vdr_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
