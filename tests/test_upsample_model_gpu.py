"""GPU: the layers on top of vdr.ops.upsample_guided on tiny networks (tests/handle_configs.py: image 32, patch 8, D = 64, 2 blocks:
a 4 x 4 grid; 7 x 7 at patch stride 4; a tiny SAM encoder for the neck output).

VitDescriptorModel.upsample_descriptors is the op applied to a contiguous copy of extract_descriptors(reshape=True), bit for bit:
at the native size, at a rectangular input size, at a patch stride below the patch, with bin=True and with facet=None.
vdr.upsample.guided on 1- and 3-channel maps equals the zero-padded call; guided_labels reproduces a label map that is constant per
guide region; AnomalyMap.upsample_guided is the guided map of d2.  pipeline.generate_features with the `upsample` key returns
feature and mask crops of equal height and width, and without the key what it returned before."""
import numpy as np
import pytest
import torch

import handle_configs as hc
from handle_configs import TINY
from oracle import sam_oracle as so
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

KW = dict(radius=2, sigma_spatial=0.9, sigma_range=0.3)


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_upsample_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return vo.make_images(TINY, 3, seed=6).cuda()


def _resized(x, h, w):
    return torch.nn.functional.interpolate(x, size=(h, w), mode="bilinear", align_corners=False).contiguous()


@pytest.mark.parametrize("setup", ((8, 32, 32, False), (8, 48, 32, False), (4, 32, 32, False), (8, 32, 32, True), (4, 40, 48, True)),
                         ids=("native", "rect48x32", "stride4", "binned", "stride4-rect-binned"))
def test_upsample_descriptors_is_the_op_on_the_extracted_map(model, images, setup):
    from vdr import ops
    stride, H, W, binned = setup
    x = images if (H, W) == (32, 32) else _resized(images, H, W)
    if (H, W) != (32, 32):
        model.set_input_size(H, W)
    model.set_patch_stride(stride)
    try:
        for facet, box, odt in (("key", None, torch.bfloat16), ("value", (3, 5, 30, 17), torch.float32)):
            got = model.upsample_descriptors(x, facet=facet, bin=binned, hierarchy=1, box=box, out_dtype=odt, **KW)
            desc = model.extract_descriptors(x, facet=facet, bin=binned, hierarchy=1, reshape=True).contiguous()
            assert tuple(desc.shape[1:3]) == ((H - 8) // stride + 1, (W - 8) // stride + 1)
            want = ops.upsample_guided(desc, x, 8, stride, box=box, out_dtype=odt, **KW)
            hb, wb = (H, W) if box is None else (box[2] - box[0], box[3] - box[1])
            assert tuple(got.shape) == (3, hb, wb, desc.shape[-1]) and got.dtype == odt
            assert torch.equal(got, want), (facet, box)
    finally:
        model.set_patch_stride(8)
        if (H, W) != (32, 32):
            model.set_input_size(32, 32)


def test_upsample_descriptors_of_the_models_own_descriptor(model, images):
    from vdr import ops
    got = model.upsample_descriptors(images, facet=None, out_dtype=torch.float32, **KW)
    desc = model.patch_embed(images).reshape(3, 4, 4, TINY.dim).contiguous()
    assert torch.equal(got, ops.upsample_guided(desc, images, 8, 8, out_dtype=torch.float32, **KW))
    # the SAM neck output
    import vdr
    cfg = so.SamCfg(img=160, patch=16, dim=64, heads=1, layers=3, mlp_hidden=128, window=4, global_idx=(1,), out_chans=64)
    sam = vdr.VitDescriptorModel(hc.sam_config(cfg), so.make_weights(cfg, seed=21), "medsam", torch.device("cuda"))
    x = so.make_images(cfg, 2, seed=3).cuda()
    got = sam.upsample_descriptors(x, facet=None, box=(40, 8, 120, 100), **KW)
    neck = sam.engine.forward(x, vdr.OUT_ENCODER, torch.float32)
    assert tuple(neck.shape) == (2, 10, 10, 64) and tuple(got.shape) == (2, 80, 92, 64) and got.dtype == torch.bfloat16
    assert torch.equal(got, ops.upsample_guided(neck.contiguous(), x, 16, 16, box=(40, 8, 120, 100), out_dtype=torch.bfloat16, **KW))


def test_guided_pads_the_channels_and_slices_them_off(images):
    from vdr import ops, upsample
    g = torch.Generator().manual_seed(4)
    for C in (1, 3):
        maps = torch.randn(3, 4, 4, C, generator=g).cuda()
        padded = torch.zeros(3, 4, 4, 8, device="cuda")
        padded[..., :C] = maps
        want = ops.upsample_guided(padded, images, 8, 8, **KW)[..., :C]
        got = upsample.guided(maps, images, 8, 8, **KW)
        assert tuple(got.shape) == (3, 32, 32, C) and torch.equal(got, want)
    flat = upsample.guided(maps[..., 0], images, 8, 8, box=(1, 2, 9, 30), **KW)
    assert tuple(flat.shape) == (3, 8, 28) and torch.equal(flat, want[:, 1:9, 2:30, 0])


def test_guided_labels_and_the_anomaly_map_follow_the_guide():
    """a guide of two flat regions whose border (column 13) is on no patch border: labels that are constant per region come back as
    the regions themselves, and a map that is constant per region comes back with the guide's edge instead of the patches'"""
    import vdr
    from vdr import upsample
    p, gh, gw = 8, 4, 4
    H = W = 32
    guide = torch.zeros(2, 3, H, W)
    guide[:, :, :, 13:] = 1.0
    guide[1] = guide[1].transpose(1, 2).clone()  # (the second image: a horizontal border)
    region = guide[:, 0].long()  # [B, H, W]
    centres = torch.arange(gh) * p + p // 2
    labels = region[:, centres][:, :, centres]  # the region of each patch centre
    labels = labels * 2 + 1  # (classes 1 and 3 of 5)
    got = upsample.guided_labels(labels.cuda(), 5, guide.cuda(), p, p, radius=2, sigma_spatial=2.0, sigma_range=0.05)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), region * 2 + 1)
    d2 = (labels.float() * 1000.25)
    amap = vdr.AnomalyMap(d2.cuda())
    up = amap.upsample_guided(guide.cuda(), radius=2, sigma_spatial=2.0, sigma_range=0.05)
    want = (region * 2 + 1).float() * 1000.25
    # (the numerator sums w_hi + w_lo, Z the fp32 w: a constant comes back to within the 2^-16 the split leaves, not exactly)
    assert tuple(up.shape) == (2, H, W) and torch.allclose(up.cpu(), want, rtol=2.0 ** -16, atol=0)
    box = up[:, 4:20, 10:18]
    assert torch.equal(amap.upsample_guided(guide.cuda(), box=(4, 10, 20, 18), radius=2, sigma_spatial=2.0, sigma_range=0.05), box)


def test_generate_features_upsampled_crops_match_the_mask_crops():
    import vdr
    from vdr import pipeline
    cfg = vo.VitCfg(96, 16, 3, 64, 1, 2, 128)
    name = "_upsample_pipe"
    vdr.ARCHS[name] = hc.vit_config(cfg)
    try:
        model = vdr.load_model(name, weights=vo.make_weights(cfg, seed=5, scale=0.05))
    finally:
        del vdr.ARCHS[name]
    rng = np.random.default_rng(8)
    H, W, S = 72, 80, 3
    img = rng.random((H, W, S, 3)).astype(np.float32)
    mask = np.zeros((H, W, S), dtype=bool)
    mask[30:41, 36:50, :] = True
    f0, m0 = pipeline.generate_features(model, img, mask, descriptor=dict(facet="key"))
    fu, mu = pipeline.generate_features(model, img, mask, max_batch=2, descriptor=dict(facet="key", upsample=dict(radius=1, sigma_range=0.2)))
    assert len(fu) == len(mu) == S
    for i in range(S):
        assert fu[i].dtype == np.float32 and fu[i].shape[2] == 64 and np.isfinite(fu[i]).all()
        assert fu[i].shape[:2] == mu[i].shape and mu[i].dtype == bool and mu[i].any()
        assert fu[i].shape[0] > f0[i].shape[0] and fu[i].shape[1] > f0[i].shape[1]  # pixels, not patches
    # without the key: what the function returned before (the default maps, the facet maps)
    fd, md = pipeline.generate_features(model, img, mask)
    fn, mn = pipeline.generate_features(model, img, mask, descriptor=None)
    for a, b, c, d in zip(fd, fn, md, mn):
        assert np.array_equal(a, b) and np.array_equal(c, d)
