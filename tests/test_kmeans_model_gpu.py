"""GPU: VitDescriptorModel.cosegment and Correspondences.points(select="kmeans") on the tiny network of
tests/test_correspondences_gpu.py (image 32, patch 8, D = 64, 2 blocks: a 4 x 4 grid; 7 x 7 at patch stride 4).

cosegment is the composition of the public pieces -- forward_descriptors, L2 normalisation, vdr.kmeans.fit(joint=True),
vdr.kmeans.vote -- bit for bit, also at a patch stride and another input size.  points(select="kmeans") returns one masked
buddy per non-empty cluster, each the top-ranked of its cluster by the restatement (tests/kmeans_ref.py restates nothing
about the model: the ranking is restated here from the returned tensors).  find_correspondences without the new keyword is
what it was."""
import numpy as np
import pytest
import torch

import handle_configs as hc
from handle_configs import TINY
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_coseg_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return vo.make_images(TINY, 3, seed=6).cuda(), vo.make_images(TINY, 3, seed=9).cuda()


def _composed(model, x, k, layer, facet, h, thresh, pct):
    import vdr
    from vdr import kmeans
    from vdr.model import minmax_normalise
    (desc,), _, (att,) = model.engine.forward_descriptors(x, [vdr.FacetOut(layer, facet, h, False, torch.bfloat16)],
                                                          maps=[vdr.AttnMap(TINY.layers - 1, 1, True)])
    sal = minmax_normalise(att[:, 0, 1:])
    rows = torch.nn.functional.normalize(desc.float(), dim=-1, eps=1e-12).to(torch.bfloat16)
    fit = kmeans.fit(rows, k, joint=True)
    labels = fit.labels.reshape(x.shape[0], -1)
    salient = kmeans.vote(labels, sal, k, thresh, pct)
    return fit, labels, salient, sal


@pytest.mark.parametrize("setup", ((8, 32), (4, 32), (8, 48)), ids=("default", "stride4", "size48"))
def test_cosegment_is_the_composition_of_its_pieces(model, images, setup):
    stride, side = setup
    x = images[0]
    if side != 32:
        x = torch.nn.functional.interpolate(x, size=(side, side), mode="bilinear", align_corners=False)
        model.set_input_size(side, side)
    model.set_patch_stride(stride)
    try:
        g = (side - 8) // stride + 1
        k = 4
        seg = model.cosegment(x, k=k, thresh=0.3, votes_percentage=60)
        fit, labels, salient, sal = _composed(model, x, k, TINY.layers - 1, "key", 0, 0.3, 60)
        assert tuple(seg.labels.shape) == (3, g, g) and seg.labels.dtype == torch.int32
        assert torch.equal(seg.labels.reshape(3, -1), labels)
        assert torch.equal(seg.kmeans.centroids, fit.centroids) and torch.equal(seg.kmeans.inertia, fit.inertia)
        assert torch.equal(seg.salient, salient) and seg.salient.dtype == torch.bool and tuple(seg.salient.shape) == (k,)
        assert torch.equal(seg.saliency.reshape(3, -1), sal)
        assert torch.equal(seg.masks, salient[seg.labels.long()])
        assert bool(seg.kmeans.converged[0]) and int(seg.kmeans.counts.sum()) == 3 * g * g
    finally:
        model.set_patch_stride(8)
        if side != 32:
            model.set_input_size(32, 32)


def test_cosegment_elbow_and_binned(model, images):
    from vdr import kmeans
    x = images[0]
    seg = model.cosegment(x, bin=True, hierarchy=1)  # (k=None: the elbow sweep)
    assert 1 <= seg.kmeans.k <= 14 and tuple(seg.salient.shape) == (seg.kmeans.k,)
    assert tuple(seg.kmeans.centroids.shape) == (1, seg.kmeans.k, 9 * 64)
    assert isinstance(seg.kmeans, kmeans.KMeans)


def test_points_by_kmeans_take_the_top_ranked_buddy_of_every_cluster(model, images):
    from vdr import kmeans
    x = images[0]
    model.set_patch_stride(4)
    try:
        c = model.find_correspondences(x, x, thresh=-1.0, keep_descriptors=True)  # (the self-match: every patch is a buddy)
        plain = model.find_correspondences(x, x, thresh=-1.0)
        assert plain.desc1 is None and plain.desc2 is None
        for f in ("nn12", "sim12", "nn21", "sim21", "saliency1", "saliency2", "mask"):
            assert torch.equal(getattr(c, f), getattr(plain, f)), f
        gw = c.grid[1]
        for b in range(2):
            a1, a2 = c.points(b, num_pairs=3), plain.points(b, num_pairs=3)
            assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])  # (select="similarity" does not look at them)
            num_pairs = 6
            idx, desc = c.buddy_descriptors(b)
            assert idx.numel() == 49 and tuple(desc.shape) == (49, 2 * c.desc1.shape[-1]) and desc.dtype == torch.bfloat16
            fit = kmeans.fit(desc, num_pairs, init="maximin")
            labels = fit.labels[0].cpu().numpy()
            rank = (c.saliency1[b][idx] * c.saliency2[b][c.nn12[b][idx].long()]).cpu().numpy()
            want = []
            for j in range(num_pairs):
                members = np.nonzero(labels == j)[0]
                if len(members):
                    want.append(members[np.argmax(rank[members])])  # (argmax: the first, i.e. lowest, position on a tie)
            want = sorted(want, key=lambda i: (-rank[i], i))
            p1, p2 = c.points(b, num_pairs=num_pairs, select="kmeans")
            assert 1 <= p1.shape[0] == len(want) <= num_pairs
            top = idx[torch.as_tensor(np.asarray(want), device=idx.device)]
            assert len(set(top.tolist())) == len(want) and bool(c.mask[b][top].all())
            want1 = torch.stack((top // gw, top % gw), 1).float() * 4 + 4.0
            j2 = c.nn12[b][top].long()
            want2 = torch.stack((j2 // gw, j2 % gw), 1).float() * 4 + 4.0
            assert torch.equal(p1, want1) and torch.equal(p2, want2)
    finally:
        model.set_patch_stride(8)
