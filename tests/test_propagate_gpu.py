"""GPU: the windowed match at model level -- VitDescriptorModel.find_correspondences(radius=) and propagate_labels on the tiny
network of tests/test_correspondences_gpu.py (image 32, patch 8, D = 64, 2 blocks: a 4 x 4 grid; 7 x 7 at patch stride 4; 4 x 6
at input size 32 x 48).

A window that covers the grid must give the global match bit for bit in every field; a small one is held to the float64
restatement (tests/local_corr_ref.py) of the bf16 descriptors of the same forward under the near-tie rule.  Propagating a
slice's labels onto itself with k = 1 returns them unchanged -- after the restatement alone has shown that every patch beats
its window neighbours by more than the bounds --, and with k = 5 the scores are vdr.knn.vote of vdr.local.topk of the op's own
cost volume."""
import numpy as np
import pytest
import torch

import handle_configs as hc
import local_corr_ref as lref
import nn_cosine_ref as nref
from handle_configs import TINY
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

N_CLASSES = 4


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_prop_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return vo.make_images(TINY, 2, seed=6).cuda(), vo.make_images(TINY, 2, seed=9).cuda()


class _Setting:
    """the model at a patch stride and an input size for the length of a with block; .grid is the grid then in force"""

    def __init__(self, model, stride=8, size=(32, 32)):
        self.model, self.stride, self.size = model, stride, size

    def __enter__(self):
        self.model.set_input_size(*self.size)
        self.model.set_patch_stride(self.stride)
        self.grid = tuple(self.model.grid)
        return self

    def __exit__(self, *exc):
        self.model.set_patch_stride(8)
        self.model.set_input_size(32, 32)


def _images_for(size, seeds=(6, 9)):
    if size == (32, 32):
        return tuple(vo.make_images(TINY, 2, seed=s).cuda() for s in seeds)
    return tuple(torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(s)).cuda() for s in seeds)


def _descriptors(model, x1, x2, h):
    """the bf16 descriptors of one forward over cat([x1, x2]), as the model's methods request them, on the CPU"""
    import vdr
    B = x1.shape[0]
    (desc,), _, _ = model.engine.forward_descriptors(torch.cat([x1, x2]), [vdr.FacetOut(TINY.layers - 1, "key", h, False, torch.bfloat16)],
                                                     maps=[])
    return desc[:B], desc[B:]


@pytest.mark.parametrize("stride,radius", ((8, 3), (4, 6), (4, 8)))
def test_a_window_that_covers_the_grid_is_the_global_match(model, images, stride, radius):
    x1, x2 = images
    with _Setting(model, stride) as s:
        assert radius >= max(s.grid) - 1
        g = model.find_correspondences(x1, x2, thresh=0.1)
        w = model.find_correspondences(x1, x2, thresh=0.1, radius=radius)
        assert g.radius is None and g.cost12 is None and w.radius == radius and w.cost12 is None and w.grid == g.grid == s.grid
        for name in ("nn12", "sim12", "nn21", "sim21", "saliency1", "saliency2", "mask"):
            assert torch.equal(getattr(g, name), getattr(w, name)), name
        assert w.nn12.dtype == torch.int32 and w.sim12.dtype == torch.float32 and w.mask.dtype == torch.bool


@pytest.mark.parametrize("stride,size,radius", ((4, (32, 32), 1), (4, (32, 32), 2), (8, (32, 48), 1)))
def test_a_small_window_against_the_restatement(model, stride, size, radius):
    from vdr import ops
    x1, x2 = _images_for(size)
    with _Setting(model, stride, size) as s:
        gh, gw = s.grid
        t = gh * gw
        c = model.find_correspondences(x1, x2, thresh=0.1, radius=radius, keep_cost=True)
        d1, d2 = _descriptors(model, x1, x2, 2)
        assert c.grid == s.grid and tuple(c.nn12.shape) == (2, t) and tuple(c.cost12.shape) == (2, t, (2 * radius + 1) ** 2)
        for a, b, sim, nn, what in ((d1, d2, c.sim12, c.nn12, "12"), (d2, d1, c.sim21, c.nn21, "21")):
            want, bnd = lref.cost(a.cpu(), b.cpu(), s.grid, radius), lref.bound(a.cpu(), b.cpu(), s.grid, radius)
            slot = lref.slot_of(nn.cpu().numpy().astype(np.int64), s.grid, radius)
            clear = nref.check_near_tie_tolerant(want, bnd, sim.cpu().numpy(), slot, f"{what} stride {stride} size {size} r {radius}")
            print(f"{what} stride {stride} size {size} r {radius}: share of clear rows {clear:.3f}")
        # the kept cost volume is the op's, on the descriptors where they lie
        cost, bs, bi = ops.local_correlation(d1, d2, s.grid, radius)
        assert torch.equal(c.cost12, cost) and torch.equal(c.sim12, bs) and torch.equal(c.nn12, bi)
        # displacement() is nn12 seen from every patch's own position, inside the window
        disp = c.displacement()
        assert disp.dtype == torch.int32 and tuple(disp.shape) == (2, gh, gw, 2) and int(disp.abs().max()) <= radius
        i = torch.arange(t, device=disp.device).view(1, gh, gw)
        back = (torch.div(i, gw, rounding_mode="floor") + disp[..., 0]) * gw + (i % gw + disp[..., 1])
        assert torch.equal(back.reshape(2, t), c.nn12.long())
        assert torch.equal(c.pixel_displacement(), disp * stride)
        nn12 = c.nn12.long()
        buddies = torch.gather(c.nn21.long(), 1, nn12) == torch.arange(t, device=nn12.device)
        assert torch.equal(c.mask, buddies & (c.saliency1 > 0.1) & (torch.gather(c.saliency2, 1, nn12) > 0.1))


def _labels(B, grid, seed=3):
    return torch.randint(0, N_CLASSES, (B,) + tuple(grid), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("stride,size,radius", ((8, (32, 32), 4), (4, (32, 32), 2), (8, (32, 48), 1)))
def test_propagating_a_slice_onto_itself_returns_its_labels(model, stride, size, radius):
    (x, _) = _images_for(size)
    with _Setting(model, stride, size) as s:
        gh, gw = s.grid
        # precondition, on the restatement alone: every patch's self-similarity beats every other candidate of its window by
        # more than the two bounds together -- for every row, no exemptions
        d, _ = _descriptors(model, x, x, 0)
        want, bnd = lref.cost(d.cpu(), d.cpu(), s.grid, radius), lref.bound(d.cpu(), d.cpu(), s.grid, radius)
        centre = want.shape[-1] // 2
        others = np.delete(want, centre, -1), np.delete(bnd, centre, -1)
        margin = (want[..., centre, None] - others[0]) - (bnd[..., centre, None] + others[1])
        print(f"stride {stride} size {size} r {radius}: smallest margin of the self-match {margin.min():.3e}, largest neighbour "
              f"cosine {others[0].max():.6f}")
        assert (margin > 0).all()
        labels = _labels(2, s.grid)
        res = model.propagate_labels(x, labels, x, N_CLASSES, radius=radius, k=1)
        assert res.grid == s.grid and res.radius == radius
        assert tuple(res.scores.shape) == (2, gh, gw, N_CLASSES) and tuple(res.idx.shape) == (2, gh * gw, 1)
        assert torch.equal(res.labels.cpu(), labels)
        assert torch.equal(res.idx[..., 0].cpu(), torch.arange(gh * gw, dtype=torch.int32).expand(2, -1))
        assert torch.equal(res.scores.cpu(), torch.nn.functional.one_hot(labels, N_CLASSES).float())


@pytest.mark.parametrize("stride,size,radius,k", ((8, (32, 32), 4, 5), (4, (32, 32), 2, 5), (8, (32, 48), 2, 5), (4, (32, 32), 8, 9)))
def test_scores_are_the_vote_of_the_top_k_of_the_ops_own_cost(model, stride, size, radius, k):
    from vdr import knn, local, ops
    x_src, x_dst = _images_for(size)
    with _Setting(model, stride, size) as s:
        gh, gw = s.grid
        labels = _labels(2, s.grid, seed=8)
        res = model.propagate_labels(x_src, labels.cuda(), x_dst, N_CLASSES, radius=radius, k=k, temperature=0.1)
        d_dst, d_src = _descriptors(model, x_dst, x_src, 0)
        cost, _, _ = ops.local_correlation(d_dst, d_src, s.grid, radius, best=False)
        idx, val = local.topk(cost, s.grid, k)
        assert torch.equal(res.idx, idx) and torch.equal(res.val, val) and torch.isfinite(val).all()
        assert torch.all(val[..., :-1] >= val[..., 1:])
        scores = knn.vote(idx, val, labels.cuda().reshape(2, gh * gw), N_CLASSES, weights="softmax", temperature=0.1)
        assert torch.equal(res.scores, scores.reshape(2, gh, gw, N_CLASSES))
        assert torch.equal(res.labels, knn.lowest_argmax(res.scores))
        # k softmax weights, each rounded once, added in fp32: 1 within (2 k) u
        assert float((res.scores.sum(-1) - 1.0).abs().max()) <= 2 * k * 2.0 ** -24
        # every neighbour lies inside the window of its patch
        lref.slot_of(idx.cpu().numpy().astype(np.int64).transpose(2, 0, 1).reshape(k * 2, gh * gw), s.grid, radius)


def test_refusals_on_the_device_model(model, images):
    x = images[0]
    labels = _labels(2, (4, 4))
    with pytest.raises(ValueError, match="labels_src"):
        model.propagate_labels(x, _labels(2, (7, 7)), x, N_CLASSES)
    with pytest.raises(ValueError, match="k must be"):
        model.propagate_labels(x, labels, x, N_CLASSES, radius=8, k=17)  # a 4 x 4 grid has 16 patches
    with pytest.raises(ValueError, match=r"0\.\.3"):
        model.propagate_labels(x, labels + 1, x, N_CLASSES)
    with pytest.raises(ValueError, match="same shape"):
        model.propagate_labels(x, labels, x[:1], N_CLASSES)
    with pytest.raises(ValueError, match="radius"):
        model.find_correspondences(x, x, radius=9)
    with _Setting(model, 4):
        with pytest.raises(ValueError, match="labels_src"):
            model.propagate_labels(x, labels, x, N_CLASSES)  # the 4 x 4 labels on the 7 x 7 grid
