"""GPU: VitDescriptorModel.find_correspondences on the tiny network of tests/golden/vit_hf_tiny.npz (image 32, patch 8,
D = 64, 2 blocks: a 4 x 4 grid; 7 x 7 at patch stride 4).

The matching is held to the float64 restatement of vdr_op_nn_cosine (tests/nn_cosine_ref.py) applied to the bf16
descriptors that forward_descriptors returns for the same inputs, with the near-tie-tolerant rule of
tests/test_nn_cosine_gpu.py; the saliency is bitwise the min-max-normalised head-mean CLS attention of
get_attention_maps; the mask and the points are restated from the returned tensors."""
import numpy as np
import pytest
import torch

import handle_configs as hc
from handle_configs import TINY
import nn_cosine_ref as nref
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_corr_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return vo.make_images(TINY, 2, seed=6).cuda(), vo.make_images(TINY, 2, seed=9).cuda()


def _minmax(a):
    lo, hi = a.min(dim=-1, keepdim=True).values, a.max(dim=-1, keepdim=True).values
    return (a - lo) / (hi - lo)


def _restated(model, x1, x2, layer, facet, h):
    """(float64 similarity, bound) of the bf16 descriptors of the same forward"""
    import vdr
    B = x1.shape[0]
    (desc,), _, _ = model.engine.forward_descriptors(torch.cat([x1, x2]), [vdr.FacetOut(layer, facet, h, False, torch.bfloat16)],
                                                     maps=[vdr.AttnMap(TINY.layers - 1, 1, True)])
    d1, d2 = desc[:B].cpu(), desc[B:].cpu()
    s = nref.similarity(d1, d2)
    return s, nref.bound(d1, d2, s)


@pytest.mark.parametrize("stride", (8, 4))
def test_an_image_against_itself(model, images, stride):
    x = images[0]
    model.set_patch_stride(stride)
    try:
        g = (32 - 8) // stride + 1
        c = model.find_correspondences(x, x)
        assert c.grid == (g, g) and c.stride == stride and c.patch == 8
        t = g * g
        for name, dt in (("nn12", torch.int32), ("nn21", torch.int32), ("sim12", torch.float32), ("sim21", torch.float32),
                         ("saliency1", torch.float32), ("saliency2", torch.float32), ("mask", torch.bool)):
            v = getattr(c, name)
            assert tuple(v.shape) == (2, t) and v.dtype == dt, name
        ident = torch.arange(t, dtype=torch.int32, device=x.device).expand(2, t)
        assert torch.equal(c.nn12, ident) and torch.equal(c.nn21, ident)
        s, b = _restated(model, x, x, TINY.layers - 1, "key", 2)
        diag_b = np.stack([np.diag(b[p]) for p in range(2)])
        for sim in (c.sim12, c.sim21):
            assert (np.abs(sim.cpu().numpy().astype(np.float64) - 1.0) <= diag_b).all()
        from vdr import ops
        assert torch.all(ops.best_buddies(c.nn12, c.nn21))
        assert torch.equal(c.saliency1, c.saliency2)
        assert torch.equal(c.mask, c.saliency1 > 0.05)
    finally:
        model.set_patch_stride(8)


@pytest.mark.parametrize("stride", (8, 4))
def test_two_images_against_the_restatement(model, images, stride):
    x1, x2 = images
    model.set_patch_stride(stride)
    try:
        c = model.find_correspondences(x1, x2, thresh=0.1)
        s, b = _restated(model, x1, x2, TINY.layers - 1, "key", 2)
        assert s.shape[1] == s.shape[2] == c.grid[0] * c.grid[1]
        nref.check_near_tie_tolerant(s, b, c.sim12.cpu().numpy(), c.nn12.cpu().numpy(), f"12 stride {stride}")
        nref.check_near_tie_tolerant(s.transpose(0, 2, 1), b.transpose(0, 2, 1), c.sim21.cpu().numpy(), c.nn21.cpu().numpy(),
                                     f"21 stride {stride}")
        att = model.get_attention_maps(torch.cat([x1, x2]), cls_only=True, head_mean=True)
        sal = _minmax(att[:, 1:])
        assert torch.equal(c.saliency1, sal[:2]) and torch.equal(c.saliency2, sal[2:])
        assert float(sal.min()) == 0.0 and float(sal.max()) == 1.0
        nn12 = c.nn12.long()
        buddies = torch.gather(c.nn21.long(), 1, nn12) == torch.arange(nn12.shape[1], device=nn12.device)
        want = buddies & (c.saliency1 > 0.1) & (torch.gather(c.saliency2, 1, nn12) > 0.1)
        assert torch.equal(c.mask, want)
    finally:
        model.set_patch_stride(8)


def test_other_facets_and_unbinned(model, images):
    x1, x2 = images
    for kw, layer, facet, h in ((dict(bin=False), TINY.layers - 1, "key", 0), (dict(facet="token", layer=0), 0, "token", 2),
                                (dict(facet="value", hierarchy=1), TINY.layers - 1, "value", 1)):
        c = model.find_correspondences(x1, x2, **kw)
        assert c.grid == (4, 4) and tuple(c.nn12.shape) == (2, 16) and tuple(c.sim21.shape) == (2, 16) and tuple(c.mask.shape) == (2, 16)
        s, b = _restated(model, x1, x2, layer, facet, h)
        assert s.shape == (2, 16, 16)
        nref.check_near_tie_tolerant(s, b, c.sim12.cpu().numpy(), c.nn12.cpu().numpy(), str(kw))


@pytest.mark.parametrize("stride", (8, 4))
def test_points_are_pixel_centres_in_descending_similarity(model, images, stride):
    x = images[0]
    model.set_patch_stride(stride)
    try:
        # thresh below every saliency: the mask is the best buddies alone (two random images may share few: the self-match
        # has them all)
        c = model.find_correspondences(x, images[1], thresh=-1.0)
        if int(c.mask.sum(1).min()) < 3:
            c = model.find_correspondences(x, x, thresh=-1.0)
        gw = c.grid[1]
        for bi in range(2):
            idx = torch.nonzero(c.mask[bi]).flatten()
            assert idx.numel() >= 3
            p1, p2 = c.points(bi, num_pairs=3)
            assert tuple(p1.shape) == (3, 2) and tuple(p2.shape) == (3, 2) and p1.dtype == torch.float32
            sims = c.sim12[bi][idx]
            top = idx[torch.sort(sims, descending=True, stable=True).indices[:3]]
            assert torch.all(c.sim12[bi][top][:-1] >= c.sim12[bi][top][1:])
            want1 = torch.stack((top // gw, top % gw), 1).float() * stride + 4.0
            j = c.nn12[bi][top].long()
            want2 = torch.stack((j // gw, j % gw), 1).float() * stride + 4.0
            assert torch.equal(p1, want1) and torch.equal(p2, want2)
            allp, _ = c.points(bi)
            assert allp.shape[0] == idx.numel()
    finally:
        model.set_patch_stride(8)


def test_mismatched_shapes_are_refused(model, images):
    with pytest.raises(ValueError, match="same shape"):
        model.find_correspondences(images[0], images[1][:1])
