"""GPU: vdr_op_local_correlation (csrc/local_corr.hip) at op level against the float64 restatement of its definition
(tests/local_corr_ref.py).

Designed inputs (nn_cosine_ref.designed: every sim a multiple of 1/16, so fp32 equals float64) must come back bit for bit in
cost, best_sim and best_idx, the -inf slots included, ties -- planted inside a window by copying rows -- resolved to the
lowest candidate.  Grids: 1x1, 1x5, 3x3, 5x7 (smaller than a panel, and than the window at r = 8); 7x15, 8x16, 9x17 (one below,
at and one above the 8 x 16 panel in each dimension); 14x14; 17x33 (three panels each way).  r in {1, 2, 4, 8}: 2, 2, 3 and 6 halo
tiles.  d in {32, 96, 448}: half a K step, a short last step, an odd number of steps through the two staging buffers.  Pairs 1
and 3; the cost == NULL and best == NULL forms.  Random inputs are held to the gathered entry-wise fp32 bound, arg-maxima to
the near-tie rule; a window that covers the grid must give vdr.ops.nn_cosine's rows bit for bit."""
import numpy as np
import pytest
import torch

import local_corr_ref as lref
import nn_cosine_ref as nref
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

GRIDS = ((1, 1), (1, 5), (3, 3), (5, 7), (7, 15), (8, 16), (9, 17), (14, 14), (17, 33))
RADII = (1, 2, 4, 8)
DIMS = (32, 96, 448)
PAIRS = 3


_CACHE = {}


def _designed(grid, d):
    """(x, y bf16 on the CPU, float64 similarity [3, t, t]) -- computed once per (grid, d), shared, never written.  Planted
    inside the windows: candidates 0 and 1, and t/2 and t/2 + 1, are copies of the queries 0 and t/2, so those queries (and
    their neighbours) meet their maximum sim = 1 twice in one window row."""
    key = ("designed", grid, d)
    if key not in _CACHE:
        gh, gw = grid
        t = gh * gw
        x, y = nref.designed(PAIRS, t, t, d, seed=100000 * gh + 1000 * gw + d)
        if gw >= 2:
            for q in (0, t // 2):
                if q % gw + 1 < gw:
                    y[:, q] = y[:, q + 1] = x[:, q]
        _CACHE[key] = (x.to(torch.bfloat16), y.to(torch.bfloat16), nref.similarity(x, y))
    return _CACHE[key]


def _want(grid, d, r):
    key = ("want", grid, d, r)
    if key not in _CACHE:
        c = lref.gather(_designed(grid, d)[2], grid, r, -np.inf)
        _CACHE[key] = (c,) + lref.best(c, grid, r)
    return _CACHE[key]


def _equal_exact(got, want, P, what):
    c, bs, bi = got
    wc, wbs, wbi, _ = want
    if c is not None:
        c = c.cpu().numpy()
        assert c.dtype == np.float32 and c.shape == wc[:P].shape, what
        assert np.array_equal(c.astype(np.float64), wc[:P]), (what, "cost", np.argwhere(c.astype(np.float64) != wc[:P])[:4].tolist())
    if bs is not None:
        bs, bi = bs.cpu().numpy(), bi.cpu().numpy()
        assert bs.dtype == np.float32 and bi.dtype == np.int32, what
        assert np.array_equal(bs.astype(np.float64), wbs[:P]), (what, "best_sim")
        assert np.array_equal(bi, wbi[:P]), (what, "best_idx", np.argwhere(bi != wbi[:P])[:4].tolist())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("grid", GRIDS)
def test_designed_inputs_are_exact(ops, grid, r, d):
    x, y, _ = _designed(grid, d)
    want = _want(grid, d, r)
    if grid[1] >= 2:  # (something to see: a maximum attained twice inside one window)
        c = want[0]
        assert ((c == c.max(-1, keepdims=True)).sum(-1) > 1).any()
    for P in (1, PAIRS):
        xd, yd = x[:P].cuda(), y[:P].cuda()
        full = ops.local_correlation(xd, yd, grid, r)
        assert tuple(full[0].shape) == (P, grid[0] * grid[1], (2 * r + 1) ** 2)
        _equal_exact(full, want, P, (grid, r, d, P, "all"))
        only_best = ops.local_correlation(xd, yd, grid, r, cost=False)
        assert only_best[0] is None
        _equal_exact(only_best, want, P, (grid, r, d, P, "cost == NULL"))
        only_cost = ops.local_correlation(xd, yd, grid, r, best=False)
        assert only_cost[1] is None and only_cost[2] is None
        _equal_exact(only_cost, want, P, (grid, r, d, P, "best == NULL"))


@pytest.mark.parametrize("grid,r", (((9, 17), 2), ((9, 17), 4), ((14, 14), 8), ((5, 7), 2)))
def test_planted_displacement(ops, grid, r):
    """Y is X's map shifted by (2, -1): the patch at (qy, qx) of X sits at (qy + 2, qx - 1) of Y, with distinct designed rows.
    best_idx is the shifted position for every query whose target is in the grid, and the displacement exactly (2, -1)."""
    gh, gw = grid
    t, d = gh * gw, 96
    rng = np.random.default_rng(77 + t)

    def draw():  # (designed()'s rows without its planted copies: 16 entries of +-1 per row)
        a = np.zeros((1, t, d), np.float32)
        for q in range(t):
            a[0, q, rng.choice(d, 16, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
        return torch.from_numpy(a)

    x, y = draw(), draw()
    i = np.arange(t)
    qy, qx = i // gw, i % gw
    ok = (qy + 2 < gh) & (qx - 1 >= 0)
    tgt = (qy + 2) * gw + (qx - 1)
    y[0, tgt[ok]] = x[0, i[ok]]
    s = nref.similarity(x, y)
    off = np.where(np.arange(t)[None, :] == np.where(ok, tgt, -1)[:, None], -np.inf, s[0])
    assert off.max() < 1.0, "the designed rows are not distinct enough: another candidate ties with the planted one"
    _, bs, bi = ops.local_correlation(x.to(torch.bfloat16).cuda(), y.to(torch.bfloat16).cuda(), grid, r, cost=False)
    bs, bi = bs.cpu().numpy()[0], bi.cpu().numpy()[0]
    assert ok.sum() > 0 and np.array_equal(bi[ok], tgt[ok]) and (bs[ok] == 1.0).all()
    assert np.array_equal(bi[ok] // gw - qy[ok], np.full(ok.sum(), 2)) and np.array_equal(bi[ok] % gw - qx[ok], np.full(ok.sum(), -1))


def _random(grid, d, P=2):
    key = ("random", grid, d, P)
    if key not in _CACHE:
        t = grid[0] * grid[1]
        gen = torch.Generator().manual_seed(11 + 1000 * grid[0] + 10 * grid[1] + d)
        _CACHE[key] = (torch.randn(P, t, d, generator=gen).to(torch.bfloat16), torch.randn(P, t, d, generator=gen).to(torch.bfloat16))
    return _CACHE[key]


@pytest.mark.parametrize("grid,r,d", (((9, 17), 4, 768), ((17, 33), 2, 96), ((5, 7), 8, 448), ((14, 14), 1, 32)))
def test_random_inputs_within_bound(ops, grid, r, d):
    x, y = _random(grid, d)
    want, b = lref.cost(x, y, grid, r), lref.bound(x, y, grid, r)
    c, bs, bi = (v.cpu().numpy() for v in ops.local_correlation(x.cuda(), y.cuda(), grid, r))
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(c), ~fin), "the -inf slots are the out-of-grid slots, no other"
    err = np.abs(c[fin].astype(np.float64) - want[fin])
    print(f"{grid} r={r} d={d}: max |cost - ref| {err.max():.3e}, max err / bound {(err / b[fin]).max():.3f}")
    assert (err <= b[fin]).all()
    slot = lref.slot_of(bi.astype(np.int64), grid, r)
    clear = nref.check_near_tie_tolerant(want, b, bs, slot, f"{grid} r={r} d={d}")
    print(f"{grid} r={r} d={d}: share of clear rows {clear:.3f}")
    assert np.array_equal(bs, np.take_along_axis(c, slot[..., None], -1)[..., 0]), "best_sim is the cost entry of best_idx"


@pytest.mark.parametrize("grid", ((5, 7), (9, 9)))
def test_window_covering_the_grid_is_nn_cosine(ops, grid):
    """r = 8 >= max(gh, gw) - 1: every candidate is in every window, so the best pair is the global one -- the same dot, the
    same association, the same comparison: vdr.ops.nn_cosine(mutual=False)'s rows bit for bit."""
    x, y = _random(grid, 96, P=3)
    xd, yd = x.cuda(), y.cuda()
    _, bs, bi = ops.local_correlation(xd, yd, grid, 8, cost=False)
    rs, ri, _, _ = ops.nn_cosine(xd, yd, mutual=False)
    assert torch.equal(bs, rs) and torch.equal(bi, ri)
    # the reverse direction, the candidate's norm multiplied first: the column side of the same global match
    _, bs, bi = ops.local_correlation(yd, xd, grid, 8, cost=False, transposed=True)
    _, _, cs, ci = ops.nn_cosine(xd, yd)
    assert torch.equal(bs, cs) and torch.equal(bi, ci)


def test_transposed_is_the_other_association(ops):
    """designed inputs are exact in either association; on random inputs the transposed cost is the transposed window of the
    plain one, bit for bit: cost_t(y, x)[j, slot(-d)] == cost(x, y)[i, slot(d)] for i = j - d"""
    grid, r, d = (9, 17), 2, 96
    x, y, _ = _designed(grid, d)
    _equal_exact(ops.local_correlation(x.cuda(), y.cuda(), grid, r, transposed=True), _want(grid, d, r), PAIRS, "designed, transposed")
    x, y = _random(grid, d)
    c = ops.local_correlation(x.cuda(), y.cuda(), grid, r, best=False)[0].cpu().numpy()
    ct = ops.local_correlation(y.cuda(), x.cuda(), grid, r, best=False, transposed=True)[0].cpu().numpy()
    j, ok = lref.window(grid[0], grid[1], r)
    WW = (2 * r + 1) ** 2
    for w in range(WW):
        q = np.nonzero(ok[:, w])[0]
        assert np.array_equal(c[:, q, w], ct[:, j[q, w], WW - 1 - w]), w


def _raw_call(x, ldx, xs, y, ldy, ys, P, grid, d, r, cost=True, best=True, fill=0xFF):
    """vdr_op_local_correlation on caller-made buffers: `work` exactly vdr_local_correlation_work_bytes inside a guarded
    allocation, the outputs with 4 guard elements on either side, all pre-filled with `fill` bytes (0xFF: NaNs).  Returns
    (cost, best_sim, best_idx) after checking every guard."""
    from vdr import _lib
    lib = _lib.load()
    dev = x.device
    t, WW = grid[0] * grid[1], (2 * r + 1) ** 2
    wb = lib.vdr_local_correlation_work_bytes(P, grid[0], grid[1], r)
    assert wb > 0 and wb % 16 == 0
    work = torch.full((wb + 512,), fill, dtype=torch.uint8, device=dev)
    outs = [torch.full(((n + 8) * 4,), fill, dtype=torch.uint8, device=dev) for n in (P * t * WW, P * t, P * t)]
    ptr = [o.data_ptr() + 16 for o in outs]
    if not cost:
        ptr[0] = None
    if not best:
        ptr[1] = ptr[2] = None
    _lib.check(lib.vdr_op_local_correlation(x.data_ptr(), ldx, xs, y.data_ptr(), ldy, ys, P, grid[0], grid[1], d, r, 0, work.data_ptr() + 256,
                                            ptr[0], ptr[1], ptr[2], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.all(work[:256] == fill) and torch.all(work[256 + wb:] == fill), "written outside work"
    for o, asked in zip(outs, (cost, best, best)):
        assert torch.all(o[:16] == fill) and torch.all(o[-16:] == fill), "written outside an output"
        assert asked or torch.all(o == fill), "an output that was not asked for was written"
    return (outs[0][16:-16].view(torch.float32).view(P, t, WW) if cost else None,
            outs[1][16:-16].view(torch.float32).view(P, t) if best else None, outs[2][16:-16].view(torch.int32).view(P, t) if best else None)


@pytest.mark.parametrize("grid,r,d", (((9, 17), 4, 96), ((5, 7), 8, 32), ((7, 15), 1, 448)))
def test_strided_views_in_place_and_work_contract(ops, grid, r, d):
    """The key facet read in place: columns [d, 2d) of a [P, 2 + t, 3d] buffer behind two prefix rows (ld = 3d) give the
    bits of the contiguous run.  Work and outputs start as NaN bytes (and as 0x00 bytes): the same bits either way, so the
    op reads nothing it has not written; nothing past work_bytes or around the outputs is touched."""
    x, y, _ = _designed(grid, d)
    want = _want(grid, d, r)
    t = grid[0] * grid[1]
    gen = torch.Generator().manual_seed(5)
    bufs = []
    for v in (x, y):
        buf = torch.randint(-3, 4, (PAIRS, 2 + t, 3 * d), generator=gen).to(torch.bfloat16)
        buf[:, 2:, d:2 * d] = v
        bufs.append(buf.cuda())
    xv, yv = bufs[0][:, 2:, d:2 * d], bufs[1][:, 2:, d:2 * d]
    for fill in (0xFF, 0x00):
        got = _raw_call(xv, 3 * d, (2 + t) * 3 * d, yv, 3 * d, (2 + t) * 3 * d, PAIRS, grid, d, r, fill=fill)
        _equal_exact(got, want, PAIRS, (grid, r, d, "raw strided", fill))
        only_best = _raw_call(xv, 3 * d, (2 + t) * 3 * d, yv, 3 * d, (2 + t) * 3 * d, PAIRS, grid, d, r, cost=False, fill=fill)
        _equal_exact(only_best, want, PAIRS, (grid, r, d, "raw strided, cost == NULL", fill))
        only_cost = _raw_call(xv, 3 * d, (2 + t) * 3 * d, yv, 3 * d, (2 + t) * 3 * d, PAIRS, grid, d, r, best=False, fill=fill)
        _equal_exact(only_cost, want, PAIRS, (grid, r, d, "raw strided, best == NULL", fill))
    _equal_exact(ops.local_correlation(xv, yv, grid, r), want, PAIRS, (grid, r, d, "ops strided"))


def test_y_at_problem_stride_zero(ops):
    """one candidate map under three query maps (expand(): stride 0) equals the three separate problems"""
    grid, r, d = (9, 17), 2, 96
    x, y, _ = _designed(grid, d)
    xd, y0 = x.cuda(), y[:1].cuda()
    got = ops.local_correlation(xd, y0.expand(PAIRS, -1, -1), grid, r)
    for p in range(PAIRS):
        one = ops.local_correlation(xd[p:p + 1], y0, grid, r)
        for g, o in zip(got, one):
            assert torch.equal(g[p:p + 1], o), p


def test_fp32_input_is_rounded_once(ops):
    grid, r, d = (7, 15), 4, 96
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 105, d, generator=gen), torch.randn(2, 105, d, generator=gen)
    a = ops.local_correlation(x.cuda(), y.cuda(), grid, r)
    b = ops.local_correlation(x.to(torch.bfloat16).cuda(), y.to(torch.bfloat16).cuda(), grid, r)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_a_problem_does_not_see_its_batch(ops):
    """random inputs: the first and the last problem of a batch of 3 have the bits of their own one-problem runs"""
    grid, r, d = (9, 17), 4, 448
    x, y = _random(grid, d, P=3)
    xd, yd = x.cuda(), y.cuda()
    got = ops.local_correlation(xd, yd, grid, r)
    for p in (0, 2):
        one = ops.local_correlation(xd[p:p + 1], yd[p:p + 1], grid, r)
        for g, o in zip(got, one):
            assert torch.equal(g[p:p + 1], o), p
