"""GPU: VitDescriptorModel.propagate_volume on a tiny ViT (tests/handle_configs.py's TINY: 2 blocks, D = 64, patch 8) at
40 x 56 images -- a 5 x 7 grid --, Z = 6 slices, n_context = 2 so the context drops slices out, index = 2 so both
directions run.

Identical slices with k = 1 return the annotation on every slice exactly; the first step with hard labels is
propagate_labels' (the same neighbours, the scores inside both bounds); the whole sweep with soft labels is held to a loop
written here from vdr.ops.local_correlation and the float64 restatement (tests/window_vote_ref.py); the result does not
depend on max_batch, the reversed volume gives the reversed result, direction="up" leaves the slices below at the
documented fill, and upsample_guided is vdr.upsample.guided + lowest_argmax."""
import numpy as np
import pytest
import torch

import handle_configs as hc
import window_vote_ref as wref
from handle_configs import TINY

pytestmark = pytest.mark.gpu

SIZE, GRID, Z, INDEX, C, RADIUS = (40, 56), (5, 7), 6, 2, 3, 2
T = GRID[0] * GRID[1]


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_volume_tiny") as m:
        m.set_input_size(*SIZE)
        assert tuple(m.grid) == GRID
        yield m


@pytest.fixture(scope="module")
def volume():
    """six slices that drift: one base image plus a growing share of a second one, and noise"""
    g = torch.Generator().manual_seed(41)
    a, b = torch.randn(3, *SIZE, generator=g), torch.randn(3, *SIZE, generator=g)
    return torch.stack([a + 0.15 * z * b + 0.05 * torch.randn(3, *SIZE, generator=g) for z in range(Z)]).cuda()


@pytest.fixture(scope="module")
def hard():
    return torch.randint(0, C, GRID, generator=torch.Generator().manual_seed(42))


@pytest.fixture(scope="module")
def soft():
    s = torch.rand(GRID + (C,), generator=torch.Generator().manual_seed(43))
    return s / s.sum(-1, keepdim=True)


def _descriptors(model, x):
    """the bf16 descriptors of one forward over x, as propagate_volume requests them"""
    import vdr
    (desc,), _, _ = model.engine.forward_descriptors(x, [vdr.FacetOut(TINY.layers - 1, "key", 0, False, torch.bfloat16)], maps=[])
    return desc


def test_identical_slices_return_the_annotation_exactly(model, volume, hard):
    from vdr import ops
    x = volume[:1].expand(Z, -1, -1, -1).contiguous()
    # precondition, on the op's own cost volume: a patch's self-match beats every other candidate of its window
    d = _descriptors(model, x[:1])
    cost = ops.local_correlation(d, d, GRID, RADIUS, best=False)[0][0]
    centre = cost.shape[-1] // 2
    others = torch.cat([cost[:, :centre], cost[:, centre + 1:]], dim=1)
    assert bool((cost[:, centre] > others.max(dim=1).values).all())
    vp = model.propagate_volume(x, hard, C, index=INDEX, radius=RADIUS, k=1, n_context=2)
    assert vp.grid == GRID and vp.radius == RADIUS and vp.index == INDEX
    assert tuple(vp.scores.shape) == (Z,) + GRID + (C,) and vp.scores.dtype == torch.float32
    assert tuple(vp.labels.shape) == (Z,) + GRID and vp.labels.dtype == torch.int64
    assert torch.equal(vp.labels.cpu(), hard.expand(Z, -1, -1))
    assert torch.equal(vp.scores.cpu(), torch.nn.functional.one_hot(hard, C).float().expand(Z, -1, -1, -1))


def test_the_first_step_is_propagate_labels(model, volume, hard):
    from vdr import ops
    k = 5
    vp = model.propagate_volume(volume, hard, C, index=INDEX, radius=RADIUS, k=k, n_context=2, direction="up")
    one = model.propagate_labels(volume[INDEX:INDEX + 1], hard[None], volume[INDEX + 1:INDEX + 2], C, radius=RADIUS, k=k, temperature=0.1)
    # the step as propagate_volume runs it: one local_correlation and one window_vote on the descriptors of the two slices
    d = _descriptors(model, volume[INDEX:INDEX + 2])
    cost = ops.local_correlation(d[1:2], d[0:1], GRID, RADIUS, best=False)[0].unsqueeze(0)
    src = torch.nn.functional.one_hot(hard, C).float().reshape(1, 1, T, C).cuda()
    scores, labels, idx, val = ops.window_vote(cost, src, GRID, k)
    assert torch.equal(idx, one.idx) and torch.equal(val, one.val)
    assert torch.equal(vp.scores[INDEX + 1].reshape(1, T, C), scores)
    want = wref.vote(cost, src, GRID, k)[0]
    both = wref.bound(cost, src, GRID, k) + wref.knn_vote_bound(val, want, "softmax", 0.1)
    assert (np.abs(scores.cpu().numpy() - one.scores.reshape(1, T, C).cpu().numpy()) <= both).all()
    clear = wref.margin_clear(want, both)
    assert np.array_equal(vp.labels[INDEX + 1].reshape(1, T).cpu().numpy()[clear], one.labels.reshape(1, T).cpu().numpy()[clear])


def _sweep_in_float64(model, x, given, index, k, n_context, temperature=0.1):
    """the sweep as the docstring states it, with the op's cost volumes (exact selection) and float64 votes: (scores
    [Z, t, C] float64, E [Z]: a bound on every entry's error -- a vote is a convex combination, so a slice's error is at most
    its sources' largest plus its own step's bound)"""
    from vdr import ops
    desc = _descriptors(model, x)
    Zn = x.shape[0]
    scores, E = np.zeros((Zn, T, C)), np.zeros(Zn)
    scores[index] = given.double().reshape(T, C).numpy()
    for order in (range(index + 1, Zn), range(index - 1, -1, -1)):
        context = []  # nearest first
        for z in order:
            sources = [index] + context[:n_context]
            S = len(sources)
            cost = ops.local_correlation(desc[z:z + 1].expand(S, -1, -1), desc[sources], GRID, RADIUS, best=False)[0].unsqueeze(0)
            src = scores[sources][None]
            scores[z] = wref.vote(cost, src, GRID, k, "softmax", temperature)[0][0]
            E[z] = max(E[s] for s in sources) + wref.bound(cost, src, GRID, k, "softmax", temperature).max()
            context.insert(0, z)
    return scores, E


def test_the_whole_sweep_against_a_loop_of_the_restatement(model, volume, soft):
    k = 5
    vp = model.propagate_volume(volume, soft, C, index=INDEX, radius=RADIUS, k=k, n_context=2)
    want, E = _sweep_in_float64(model, volume, soft, INDEX, k, 2)
    got = vp.scores.reshape(Z, T, C).cpu().numpy()
    assert np.array_equal(got[INDEX], soft.reshape(T, C).numpy())  # what was given
    for z in range(Z):
        err = np.abs(got[z] - want[z]).max()
        print(f"slice {z}: largest error {err:.3e}, bound {E[z]:.3e}")
        assert err <= E[z]
    from vdr import knn
    assert torch.equal(vp.labels, knn.lowest_argmax(vp.scores))
    assert float((vp.scores.sum(-1) - 1.0).abs().max()) < 1e-5


def test_the_result_does_not_depend_on_max_batch(model, volume, soft):
    a = model.propagate_volume(volume, soft, C, index=INDEX, radius=RADIUS, k=5, n_context=2, max_batch=2)
    b = model.propagate_volume(volume, soft, C, index=INDEX, radius=RADIUS, k=5, n_context=2, max_batch=5)
    assert torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)


def test_the_reversed_volume_gives_the_reversed_result(model, volume, soft):
    a = model.propagate_volume(volume, soft, C, index=INDEX, radius=RADIUS, k=5, n_context=2, max_batch=4)
    b = model.propagate_volume(volume.flip(0), soft, C, index=Z - 1 - INDEX, radius=RADIUS, k=5, n_context=2, max_batch=4)
    assert b.index == Z - 1 - INDEX
    assert torch.equal(a.scores, b.scores.flip(0)) and torch.equal(a.labels, b.labels.flip(0))


def test_one_direction_leaves_the_other_side_at_the_fill(model, volume, hard):
    both = model.propagate_volume(volume, hard, C, index=INDEX, radius=RADIUS, k=5, n_context=2)
    up = model.propagate_volume(volume, hard, C, index=INDEX, radius=RADIUS, k=5, n_context=2, direction="up")
    down = model.propagate_volume(volume, hard, C, index=INDEX, radius=RADIUS, k=5, n_context=2, direction="down")
    assert "scores 0 and labels -1" in " ".join(type(up).__doc__.split())  # the fill is documented
    assert torch.equal(up.scores[INDEX:], both.scores[INDEX:]) and torch.equal(up.labels[INDEX:], both.labels[INDEX:])
    assert bool((up.scores[:INDEX] == 0).all()) and bool((up.labels[:INDEX] == -1).all())
    assert torch.equal(down.scores[:INDEX + 1], both.scores[:INDEX + 1]) and torch.equal(down.labels[:INDEX + 1], both.labels[:INDEX + 1])
    assert bool((down.scores[INDEX + 1:] == 0).all()) and bool((down.labels[INDEX + 1:] == -1).all())
    # n_context = 0: every slice from the annotated one alone, so the order of the slices on one side does not matter
    lone = model.propagate_volume(volume, hard, C, index=INDEX, radius=RADIUS, k=5, n_context=0)
    swapped = model.propagate_volume(volume[[0, 1, 2, 5, 4, 3]], hard, C, index=INDEX, radius=RADIUS, k=5, n_context=0)
    assert torch.equal(lone.scores[[0, 1, 2, 5, 4, 3]], swapped.scores)


def test_upsample_guided_is_guided_and_lowest_argmax(model, volume, soft):
    from vdr import knn, upsample
    vp = model.propagate_volume(volume, soft, C, index=INDEX, radius=RADIUS, k=5, n_context=2)
    got = vp.upsample_guided(volume)
    assert tuple(got.shape) == (Z,) + SIZE and got.dtype == torch.int64
    by_hand = upsample.guided(vp.scores, volume, TINY.patch, TINY.patch, out_dtype=torch.float32)
    assert torch.equal(got, knn.lowest_argmax(by_hand))
    box = (8, 16, 32, 48)
    assert torch.equal(vp.upsample_guided(volume, box=box),
                       knn.lowest_argmax(upsample.guided(vp.scores, volume, TINY.patch, TINY.patch, box=box, out_dtype=torch.float32)))
