"""GPU: vdr_op_nn_cosine (csrc/nn_cosine.hip) at op level against the float64 restatement of its definition
(tests/nn_cosine_ref.py).

Designed inputs (exactly 16 entries of +-1 per row: rn = 0.25, every sim a multiple of 1/16) must come back bit for bit in
all four outputs, ties -- planted and incidental -- resolved to the lowest index.  X and Y are drawn differently, so a
row / column swap of the accumulator layout shows.  Shapes (tx, ty): (1, 1), (5, 3), (127, 129), (128, 128), (130, 257): the
ragged last panel and tile on each side, more than one panel with more than one tile.  d: 32 (half a K step: one short
step), 96 (a short last step), 448 (7 K steps: an odd number through the two staging buffers); 768 with random inputs.
Pairs: 1 and 3.  Random inputs are held to the entry-wise fp32 bound of the restatement, arg-maxima with the near-tie rule."""
import numpy as np
import pytest
import torch

import nn_cosine_ref as nref
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (5, 3), (127, 129), (128, 128), (130, 257))
DIMS = (32, 96, 448)
PAIRS = 3


_CACHE = {}


def _designed(tx, ty, d):
    """(x, y bf16 on the CPU, float64 similarity, its nearest()) of 3 pairs -- computed once per shape, shared, never written"""
    key = ("designed", tx, ty, d)
    if key not in _CACHE:
        x, y = nref.designed(PAIRS, tx, ty, d, seed=10000 * tx + 10 * ty + d)
        s = nref.similarity(x, y)
        _CACHE[key] = (x.to(torch.bfloat16), y.to(torch.bfloat16), s, nref.nearest(s))
    return _CACHE[key]


def _random(tx, ty, d):
    key = ("random", tx, ty, d)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(7 + 10000 * tx + 10 * ty + d)
        x = torch.randn(2, tx, d, generator=gen).to(torch.bfloat16)
        y = (torch.randn(2, ty, d, generator=gen) * 3).to(torch.bfloat16)
        s = nref.similarity(x, y)
        _CACHE[key] = (x, y, s, nref.bound(x, y, s))
    return _CACHE[key]


def _equal_exact(got, want, P, what):
    rs, ri, cs, ci = (t.cpu().numpy() for t in got)
    wrs, wri, wcs, wci = (w[:P] for w in want)
    assert ri.dtype == np.int32 and ci.dtype == np.int32 and rs.dtype == np.float32 and cs.dtype == np.float32
    assert np.array_equal(rs.astype(np.float64), wrs), (what, "row_sim")
    assert np.array_equal(ri, wri), (what, "row_idx", np.argwhere(ri != wri)[:4].tolist())
    assert np.array_equal(cs.astype(np.float64), wcs), (what, "col_sim")
    assert np.array_equal(ci, wci), (what, "col_idx", np.argwhere(ci != wci)[:4].tolist())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_designed_inputs_are_exact(ops, shape, d):
    tx, ty = shape
    x, y, s, want = _designed(tx, ty, d)
    if tx >= 100:  # (something to see: maxima attained more than once, on both sides)
        assert nref.rows_with_ties(s) > 1 and nref.rows_with_ties(s.transpose(0, 2, 1)) > 1
    for P in (1, PAIRS):
        got = ops.nn_cosine(x[:P].cuda(), y[:P].cuda())
        assert tuple(got[0].shape) == (P, tx) and tuple(got[3].shape) == (P, ty)
        _equal_exact(got, want, P, (shape, d, P))


def _raw_call(x, ldx, xs, tx, y, ldy, ys, ty, P, d, mutual=True):
    """vdr_op_nn_cosine on caller-made buffers: outputs with 4 guard elements on either side, the work buffer exactly
    vdr_nn_cosine_work_bytes inside a guarded allocation.  Returns the four outputs after checking every guard."""
    from vdr import _lib
    lib = _lib.load()
    dev = x.device
    wb = lib.vdr_nn_cosine_work_bytes(P, tx, ty)
    work = torch.full((wb + 512,), 0xA5, dtype=torch.uint8, device=dev)
    outs = [torch.full((P * t + 8,), fill, dtype=dt, device=dev)
            for t, dt, fill in ((tx, torch.float32, -7.0), (tx, torch.int32, -7), (ty, torch.float32, -7.0), (ty, torch.int32, -7))]
    ptr = [o.data_ptr() + 16 for o in outs]
    if not mutual:
        ptr[2] = ptr[3] = None
    _lib.check(lib.vdr_op_nn_cosine(x.data_ptr(), ldx, xs, tx, y.data_ptr(), ldy, ys, ty, P, d, work.data_ptr() + 256, ptr[0], ptr[1],
                                    ptr[2], ptr[3], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.all(work[:256] == 0xA5) and torch.all(work[256 + wb:] == 0xA5)
    for o in outs:
        assert torch.all(o[:4] == -7) and torch.all(o[-4:] == -7)
    if not mutual:
        assert torch.all(outs[2] == -7) and torch.all(outs[3] == -7)
    return [o[4:-4].view(P, -1) for o in outs]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_strided_views_in_place_and_sentinels(ops, shape, d):
    """The same data as columns [d, 2d) of a [P, 2 + t, 3d] buffer behind two prefix rows (ld = 3d): the bits of the
    contiguous run; guards around the outputs and the work buffer untouched."""
    tx, ty = shape
    x, y, _, want = _designed(tx, ty, d)
    gen = torch.Generator().manual_seed(5)
    bufs = []
    for t, v in ((tx, x), (ty, y)):
        buf = torch.randint(-3, 4, (PAIRS, 2 + t, 3 * d), generator=gen).to(torch.bfloat16)
        buf[:, 2:, d:2 * d] = v
        bufs.append(buf.cuda())
    xv, yv = bufs[0][:, 2:, d:2 * d], bufs[1][:, 2:, d:2 * d]
    got = _raw_call(xv, 3 * d, (2 + tx) * 3 * d, tx, yv, 3 * d, (2 + ty) * 3 * d, ty, PAIRS, d)
    _equal_exact(got, want, PAIRS, (shape, d, "raw strided"))
    # ... and through the Python surface, which reads the views where they lie
    _equal_exact(ops.nn_cosine(xv, yv), want, PAIRS, (shape, d, "ops strided"))
    rows_only = _raw_call(xv, 3 * d, (2 + tx) * 3 * d, tx, yv, 3 * d, (2 + ty) * 3 * d, ty, PAIRS, d, mutual=False)
    assert torch.equal(rows_only[0], got[0]) and torch.equal(rows_only[1], got[1])


@pytest.mark.parametrize("shape", ((5, 3), (130, 257)))
def test_a_broadcast_map_equals_its_materialised_copies(ops, shape):
    tx, ty = shape
    d = 96
    x, y, _, _ = _designed(tx, ty, d)
    x1, yc = x[:1].cuda(), y.cuda()
    want = ops.nn_cosine(x1.expand(PAIRS, tx, d).contiguous(), yc)
    got = ops.nn_cosine(x1.expand(PAIRS, tx, d), yc)
    raw = _raw_call(x1, d, 0, tx, yc, d, ty * d, ty, PAIRS, d)
    for g, r, w in zip(got, raw, want):
        assert torch.equal(g, w) and torch.equal(r, w)
    # the other side broadcast
    y1 = y[1:2].cuda()
    for g, w in zip(ops.nn_cosine(x.cuda(), y1.expand(PAIRS, ty, d)), ops.nn_cosine(x.cuda(), y1.expand(PAIRS, ty, d).contiguous())):
        assert torch.equal(g, w)


@pytest.mark.parametrize("d", DIMS + (768,))
@pytest.mark.parametrize("shape", SHAPES)
def test_random_inputs_within_the_bound(ops, shape, d):
    tx, ty = shape
    x, y, s, b = _random(tx, ty, d)
    rs, ri, cs, ci = (t.cpu().numpy() for t in ops.nn_cosine(x.cuda(), y.cuda()))
    clear_r = nref.check_near_tie_tolerant(s, b, rs, ri, f"rows {shape} d={d}")
    clear_c = nref.check_near_tie_tolerant(s.transpose(0, 2, 1), b.transpose(0, 2, 1), cs, ci, f"cols {shape} d={d}")
    # the arg-max check is a real one: for at least half of the rows the float64 best-to-second gap exceeds the bound
    assert clear_r >= 0.5 and clear_c >= 0.5, (clear_r, clear_c)
    # fp32 inputs are rounded once to bf16: the same bits
    for g, w in zip(ops.nn_cosine(x.float().cuda(), y.float().cuda()), (rs, ri, cs, ci)):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("shape", ((5, 3), (130, 257)))
def test_batch_independence_and_reproducibility(ops, shape):
    tx, ty = shape
    for d in (96, 768):
        x, y, _, _ = _random(tx, ty, d)
        x3, y3 = torch.cat([x, x[:1]]).cuda(), torch.cat([y, y[:1]]).cuda()
        three = ops.nn_cosine(x3, y3)
        again = ops.nn_cosine(x3, y3)
        one = ops.nn_cosine(x3[1:2], y3[1:2])
        rows = ops.nn_cosine(x3, y3, mutual=False)
        assert rows[2] is None and rows[3] is None
        for k in range(4):
            assert torch.equal(three[k], again[k]), (shape, d, k)
            assert torch.equal(three[k][1:2], one[k]), (shape, d, k)
            assert torch.equal(three[k][2], three[k][0]), (shape, d, k)
        assert torch.equal(rows[0], three[0]) and torch.equal(rows[1], three[1])


def test_many_pairs_take_the_unsplit_path_and_few_pairs_the_split_one(ops):
    """The launch splits Y's tiles over more workgroups when there are few (pair, panel) items; the fold of the partial
    maxima is order-independent, so 600 copies of one pair (no split) give the bits of the single pair (split)."""
    x, y, _, want = _designed(130, 257, 32)
    one = ops.nn_cosine(x[:1].cuda(), y[:1].cuda())
    many = ops.nn_cosine(x[:1].cuda().expand(600, 130, 32), y[:1].cuda().expand(600, 257, 32))
    _equal_exact(one, want, 1, "one pair")
    for k in range(4):
        assert torch.equal(many[k], one[k].expand_as(many[k])), k


def test_refusals_leave_the_outputs_alone(ops):
    from vdr import _lib
    lib = _lib.load()
    x = torch.ones(1, 4, 64, dtype=torch.bfloat16, device="cuda")
    y = torch.ones(1, 3, 64, dtype=torch.bfloat16, device="cuda")
    work = torch.zeros(lib.vdr_nn_cosine_work_bytes(1, 4, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((64,), -3.0, device="cuda")
    idx = torch.full((64,), -3, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(x=x.data_ptr(), ldx=64, tx=4, y=y.data_ptr(), ldy=64, ty=3, d=64, work=work.data_ptr(), ci=idx.data_ptr() + 64):
        return lib.vdr_op_nn_cosine(x, ldx, 0, tx, y, ldy, 0, ty, 1, d, work, out.data_ptr(), idx.data_ptr(), out.data_ptr() + 64, ci, s)

    assert call(d=48, ldx=48, ldy=48) == -7
    for kw in (dict(x=None), dict(ldx=32), dict(tx=0), dict(ci=None), dict(x=x.data_ptr() + 2), dict(work=work.data_ptr() + 4), dict(ldy=68)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(out == -3.0) and torch.all(idx == -3)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.all(out[:4] == 1.0) and torch.all(out[16:19] == 1.0) and torch.all(idx[:4] == 0) and torch.all(idx[16:19] == 0)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.nn_cosine(torch.ones(1, 4, 48, dtype=torch.bfloat16, device="cuda"), torch.ones(1, 3, 48, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError, match="agree"):
        ops.nn_cosine(x, torch.ones(2, 3, 64, dtype=torch.bfloat16, device="cuda"))
