"""GPU: vdr_op_window_vote (csrc/window_vote.hip) through vdr.ops.window_vote.

Designed inputs come back bit for bit in all four outputs: the selection is exact comparisons for any cost values, and the
scores are exact where every weight is exactly 1 or 0 (costs from {0, 2, 4} at T = 0.01: exp(-200) underflows), where all
costs are equal (1 / k each), with uniform weights, and with one-hot or dyadic src (sums of multiples of 1/8 are exact, and
one correctly rounded division of two exact numbers is one number).  Random inputs are held to the float64 restatement
inside the bound of tests/window_vote_ref.py; a problem's bits do not depend on the batch; null outputs change nothing else;
and the op equals vdr.local.vote_window on the device."""
import numpy as np
import pytest
import torch

import window_vote_ref as wref
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

# (S, grid, r, k, C, P): every grid, radius, source count and class count of the edges, k = 1, 5, 16 and the corner maximum
# S * min(gh, r + 1) * min(gw, r + 1) (marked *), one and three problems; the last row is the widest (2312 floats)
SHAPES = ((1, (1, 1), 1, 1, 1, 1),     # * one patch, one candidate
          (8, (1, 1), 8, 8, 2, 3),     # * one patch, eight sources
          (2, (2, 3), 1, 8, 5, 1),     # *
          (1, (2, 3), 4, 6, 2, 3),     # * the window covers the grid
          (2, (2, 3), 8, 12, 64, 1),   # *
          (8, (2, 3), 8, 16, 5, 3),
          (1, (5, 7), 1, 4, 1, 3),     # *
          (8, (5, 7), 1, 5, 2, 1),
          (2, (5, 7), 4, 16, 64, 3),
          (1, (5, 7), 8, 16, 5, 1),
          (2, (9, 17), 4, 5, 1, 3),
          (1, (9, 17), 1, 1, 64, 1),
          (8, (9, 17), 8, 16, 5, 1))
DESIGNS = ("weights_0_or_1", "weights_0_or_1_one_hot", "all_equal", "uniform")


def _design(name, S, grid, r, C, P):
    """(cost, src, weights, temperature) of a design"""
    if name == "all_equal":
        cost, src = wref.designed(P, S, grid, r, C, seed=4, values=(0.5,))
        return cost, src, "softmax", 0.1
    cost, src = wref.designed(P, S, grid, r, C, seed=5, dyadic=name != "weights_0_or_1_one_hot")
    return (cost, src, "uniform", 0.1) if name == "uniform" else (cost, src, "softmax", 0.01)


def _run(ops, cost, src, grid, k, **kw):  # noqa: F811
    out = ops.window_vote(cost.cuda(), src.cuda(), grid, k, **kw)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu() for o in out)


@pytest.mark.parametrize("design", DESIGNS)
@pytest.mark.parametrize("S,grid,r,k,C,P", SHAPES)
def test_designed_inputs_come_back_bit_for_bit(ops, S, grid, r, k, C, P, design):  # noqa: F811
    cost, src, weights, T = _design(design, S, grid, r, C, P)
    scores, labels, idx, val = _run(ops, cost, src, grid, k, weights=weights, temperature=T)
    t = grid[0] * grid[1]
    assert scores.dtype == torch.float32 and labels.dtype == torch.int32 and idx.dtype == torch.int32 and val.dtype == torch.float32
    assert tuple(scores.shape) == (P, t, C) and tuple(labels.shape) == (P, t) and tuple(idx.shape) == tuple(val.shape) == (P, t, k)
    want, _, want_idx, want_val = wref.vote(cost, src, grid, k, weights, T)
    want = want.astype(np.float32)  # (exact: see the module docstring; the labels are those of the rounded scores)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(val.numpy().astype(np.float64), want_val)
    assert np.array_equal(scores.numpy(), want)
    assert np.array_equal(labels.numpy(), want.argmax(-1))
    if design == "all_equal":  # the k first candidates in (source, slot) order, each weighing 1 / k
        assert (val == 0.5).all() and (np.diff(wref.select(cost, grid, k)[0], axis=-1) > 0).all()


@pytest.mark.parametrize("weights,T", (("softmax", 0.1), ("softmax", 0.01), ("uniform", 0.1)))
@pytest.mark.parametrize("S,grid,r,k,C,P", ((1, (5, 7), 4, 5, 2, 3), (8, (9, 17), 8, 16, 8, 1), (2, (27, 27), 4, 5, 8, 2), (3, (2, 3), 1, 7, 64, 3)))
def test_random_inputs_against_the_restatement(ops, S, grid, r, k, C, P, weights, T):  # noqa: F811
    cost, src = wref.random_inputs(P, S, grid, r, C, seed=13 + S)
    scores, labels, idx, val = _run(ops, cost, src, grid, k, weights=weights, temperature=T)
    want, want_lab, want_idx, want_val = wref.vote(cost, src, grid, k, weights, T)
    bnd = wref.bound(cost, src, grid, k, weights, T)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(val.numpy().astype(np.float64), want_val)
    ratio = np.abs(scores.numpy() - want) / bnd
    clear = wref.margin_clear(want, bnd)
    print(f"S {S} grid {grid} r {r} k {k} C {C} P {P} {weights} T {T}: worst error / bound {ratio.max():.3f}, clear rows {clear.mean():.4f}")
    assert (ratio <= 1.0).all()
    assert np.array_equal(labels.numpy()[clear], want_lab[clear]) and clear.mean() > 0.9


@pytest.mark.parametrize("S,grid,r,k,C", ((1, (5, 7), 4, 5, 3), (8, (9, 17), 8, 16, 5), (2, (2, 3), 1, 8, 64)))
def test_a_problem_does_not_depend_on_its_batch(ops, S, grid, r, k, C):  # noqa: F811
    cost, src = wref.random_inputs(3, S, grid, r, C, seed=17)
    whole = _run(ops, cost, src, grid, k)
    for p in range(3):
        alone = _run(ops, cost[p:p + 1], src[p:p + 1], grid, k)
        for a, b, name in zip(whole, alone, ("scores", "labels", "idx", "val")):
            assert torch.equal(a[p:p + 1], b), (p, name)


@pytest.mark.parametrize("weights", ("softmax", "uniform"))
def test_null_outputs_change_nothing_else(ops, weights):  # noqa: F811
    S, grid, r, k, C = 3, (5, 7), 2, 5, 4
    cost, src = wref.random_inputs(2, S, grid, r, C, seed=19)
    scores, labels, idx, val = _run(ops, cost, src, grid, k, weights=weights)
    s1, l1, i1, v1 = _run(ops, cost, src, grid, k, weights=weights, labels=False)
    assert l1 is None and torch.equal(s1, scores) and torch.equal(i1, idx) and torch.equal(v1, val)
    s2, l2, i2, v2 = _run(ops, cost, src, grid, k, weights=weights, neighbours=False)
    assert i2 is None and v2 is None and torch.equal(s2, scores) and torch.equal(l2, labels)
    s3, l3, i3, v3 = _run(ops, cost, src, grid, k, weights=weights, labels=False, neighbours=False)
    assert l3 is None and i3 is None and v3 is None and torch.equal(s3, scores)


@pytest.mark.parametrize("S,grid,r,k,C,P", ((1, (5, 7), 4, 5, 2, 3), (8, (9, 17), 8, 16, 8, 1), (4, (27, 27), 4, 5, 2, 1)))
def test_the_op_equals_the_torch_statement_on_the_device(ops, S, grid, r, k, C, P):  # noqa: F811
    from vdr import local
    cost, src = wref.random_inputs(P, S, grid, r, C, seed=23)
    cost, src = cost.cuda(), src.cuda()
    for weights in ("softmax", "uniform"):
        scores, labels, idx, val = ops.window_vote(cost, src, grid, k, weights=weights)
        t_scores, t_labels, t_idx, t_val = local.vote_window(cost, src, grid, k, weights=weights)
        assert torch.equal(idx, t_idx) and torch.equal(val, t_val) and torch.equal(labels, t_labels)
        # the two differ by their exponentials alone: both are inside the bound of the restatement
        bnd = torch.from_numpy(wref.bound(cost, src, grid, k, weights, 0.1)).cuda()
        assert bool(((scores.double() - t_scores.double()).abs() <= 2.0 * bnd).all())
        if weights == "uniform":
            assert torch.equal(scores, t_scores)


def test_a_cost_volume_of_local_correlation_is_taken_as_written(ops):  # noqa: F811
    """the -inf of the slots outside the grid, and S cost volumes of one expand()ed target, straight from the other op"""
    grid, r, S, C, k = (5, 7), 2, 3, 4, 5
    g = torch.Generator().manual_seed(29)
    target = torch.randn(1, 35, 64, generator=g).bfloat16().cuda()
    sources = torch.randn(S, 35, 64, generator=g).bfloat16().cuda()
    cost, _, _ = ops.local_correlation(target.expand(S, -1, -1), sources, grid, r, best=False)
    _, src = wref.random_inputs(1, S, grid, r, C, seed=31)
    scores, labels, idx, val = _run(ops, cost.unsqueeze(0), src, grid, k)
    want, want_lab, want_idx, want_val = wref.vote(cost.unsqueeze(0), src, grid, k)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(val.numpy().astype(np.float64), want_val)
    assert (np.abs(scores.numpy() - want) <= wref.bound(cost.unsqueeze(0), src, grid, k)).all()
