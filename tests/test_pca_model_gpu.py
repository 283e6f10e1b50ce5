"""GPU: vdr.pca.fit / transform, vdr.pca_colorize and VitDescriptorModel.pca_descriptors.

The fit and the colour maps are held to the golden files of sklearn and of the reference's own pca_colorize
(tests/golden/README_pca.md) inside the gates the CPU restatement is held to (tests/pca_ref.py: 4 x what it measured).  On the
tiny network of tests/golden/vit_hf_tiny.npz (image 32, patch 8, D = 64, 2 blocks) pca_descriptors must be, bit for bit,
pca_colorize of the rows the model's dense output / extract_descriptors returns -- image by image, and of the concatenated
rows when joint -- at the default grid, at patch stride 4 and at another input size."""
import numpy as np
import pytest
import torch

import handle_configs as hc
import pca_ref as pref
from handle_configs import TINY
from ops_checks import assert_same_bits
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_pca_tiny") as m:
        yield m


@pytest.mark.parametrize("name", pref.SK_CASES)
def test_fit_and_transform_against_sklearn(golden_dir, name):
    import vdr
    g, x = pref.load_golden(golden_dir, name)
    xd = x.cuda()
    p = vdr.pca.fit(xd, 3)
    assert p.mean.shape == (1, x.shape[1]) and p.components.shape == (1, 3, x.shape[1]) and p.components.dtype == torch.float32
    comps = p.components[0].cpu().numpy()
    cos = 1 - pref.component_cosine(comps, g["components"])
    ev = np.abs(p.explained_variance[0].cpu().numpy() - g["explained_variance"]) / g["explained_variance"]
    evr = np.abs(p.explained_variance_ratio[0].cpu().numpy() - g["explained_variance_ratio"]) / g["explained_variance_ratio"]
    rgb = p.transform(xd, scale=True).cpu().numpy().astype(np.float64)
    assert rgb.shape == (x.shape[0], 3)
    err = np.abs(rgb - g["rgb_full"]).max()
    print(name, "1-|cos|", cos.max(), "explained variance", ev.max(), "ratio", evr.max(), "rgb", err)
    assert np.all((comps * g["components"]).sum(-1) > 0)
    assert cos.max() <= pref.GATE_COS and ev.max() <= pref.GATE_EV and evr.max() <= pref.GATE_RATIO and err <= pref.GATE_RGB
    raw = p.transform(xd).cpu().numpy().astype(np.float64)
    assert np.abs((raw - raw.min()) / (raw.max() - raw.min()) - rgb).max() <= 2e-7  # (scale=True is the same projection, rescaled)


def test_pca_colorize_against_the_references_maps(golden_dir):
    import vdr
    g, x = pref.load_golden(golden_dir, "pca_ref_colorize")
    rgb = vdr.pca_colorize(x.numpy(), (32, 32))
    bg = vdr.pca_colorize(x.numpy(), (32, 32), remove_bg=True)
    assert isinstance(rgb, np.ndarray) and rgb.shape == (32, 32, 3) and rgb.dtype == np.float32
    e0, e1 = np.abs(rgb - g["rgb"]).max(), np.abs(bg - g["rgb_remove_bg"]).max()
    print("pca_colorize", e0, "remove_bg", e1)
    assert np.array_equal(bg[..., 0] > 0, g["mask"])  # (the masked map is zero off the mask, and above the cut on it)
    assert e0 <= pref.GATE_REF_RGB and e1 <= pref.GATE_REF_RGB
    t = vdr.pca_colorize(x.cuda(), (32, 32))
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), rgb)
    for name in pref.SK_CASES[:1]:
        g, x = pref.load_golden(golden_dir, name)
        out = vdr.pca_colorize(x.numpy(), (8, 8))
        assert np.abs(out.reshape(64, 3) - g["rgb_default"]).max() <= pref.GATE_RGB


def _check(model, x, grid):
    import vdr
    gh, gw = grid
    B = x.shape[0]
    assert tuple(model.grid) == grid
    dense = model.patch_embed(x)  # what get_dense_descriptor returns for this model
    key = model.extract_descriptors(x, facet="key")[:, 0]
    for rows, kw in ((dense, {}), (key, dict(facet="key")), (key, dict(facet="key", layer=TINY.layers - 1))):
        got = model.pca_descriptors(x, **kw)
        assert got.shape == (B, gh, gw, 3) and got.dtype == torch.float32
        for b in range(B):
            assert_same_bits(got[b], vdr.pca_colorize(rows[b], (gh, gw)), ("per image", kw, b))
        joint = model.pca_descriptors(x, joint=True, **kw)
        assert_same_bits(joint, vdr.pca_colorize(rows.reshape(B * gh * gw, -1), (B, gh, gw)), ("joint", kw))
    bg = model.pca_descriptors(x, remove_bg=True)
    for b in range(B):
        assert_same_bits(bg[b], vdr.pca_colorize(dense[b], (gh, gw), remove_bg=True), ("remove_bg", b))
    k5 = model.pca_descriptors(x, n_components=5)
    assert k5.shape == (B, gh, gw, 5) and float(k5.min()) == 0.0 and float(k5.max()) == 1.0


def test_pca_descriptors_is_pca_colorize_of_the_models_rows(model):
    _check(model, vo.make_images(TINY, 3, seed=6).cuda(), (4, 4))


def test_pca_descriptors_follows_the_patch_stride_and_the_input_size(model):
    x = vo.make_images(TINY, 2, seed=7).cuda()
    model.set_patch_stride(4)
    try:
        _check(model, x, (7, 7))
    finally:
        model.set_patch_stride(8)
    big = torch.nn.functional.interpolate(x, size=(48, 40), mode="bilinear", align_corners=False)
    model.set_input_size(48, 40)
    try:
        _check(model, big, (6, 5))
    finally:
        model.set_input_size(32, 32)


def test_refusals_come_before_any_device_work(model):
    x = vo.make_images(TINY, 1, seed=6)  # (on the host: nothing below gets as far as moving it)
    for kw, msg in ((dict(facet="keys"), "facet"), (dict(facet="key", layer=2), "out of range"), (dict(layer=1), "needs a facet"),
                    (dict(n_components=0), "n_components"), (dict(n_components=9), "n_components")):
        with pytest.raises(ValueError, match=msg):
            model.pca_descriptors(x, **kw)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        model.pca_descriptors(x[0])


def test_pca_descriptors_of_a_sam_encoder_is_pca_colorize_of_its_neck_output():
    """window > 0: the dense descriptor is the conv-neck output (what get_dense_descriptor returns for 'medsam'), fp32,
    channel-last on the device; a 14 x 14 grid of 64 channels"""
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(img=224, patch=16, dim=128, heads=2, layers=2, mlp_hidden=256, window=7, global_idx=(1,), out_chans=64)
    vdr.ARCHS["_pca_sam"] = hc.sam_config(cfg)
    try:
        m = vdr.load_model("_pca_sam", weights=so.make_weights(cfg, seed=21, scale=0.05))
    finally:
        del vdr.ARCHS["_pca_sam"]
    x = so.make_images(cfg, 2, seed=22).cuda()
    rows = m.image_encoder(x).permute(0, 2, 3, 1).reshape(2, 196, 64).contiguous()
    got = m.pca_descriptors(x)
    assert got.shape == (2, 14, 14, 3) and got.dtype == torch.float32
    for b in range(2):
        assert_same_bits(got[b], vdr.pca_colorize(rows[b], (14, 14)), ("per image", b))
        assert_same_bits(m.pca_descriptors(x, remove_bg=True)[b], vdr.pca_colorize(rows[b], (14, 14), remove_bg=True), ("remove_bg", b))
    assert_same_bits(m.pca_descriptors(x, joint=True), vdr.pca_colorize(rows.reshape(392, 64), (2, 14, 14)), "joint")
    with pytest.raises(ValueError):
        m.pca_descriptors(x, facet="key")  # (extract_descriptors' own refusal of SAM models)


@pytest.mark.parametrize("d", (256, 768))
def test_a_fit_does_not_depend_on_the_batch_it_came_in(d):
    """at these widths the batched eigen-solver and a single call take different routes on the build this was written
    against: a lone problem, and one in a batch of two, must still get the components they get inside a batch of three"""
    import vdr
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(3, 300, d, generator=g) * torch.linspace(4, 0.2, d) + torch.randn(d, generator=g)).to(torch.bfloat16).cuda()
    whole = vdr.pca.fit(x, 3)
    for sl in (slice(0, 1), slice(1, 2), slice(2, 3), slice(1, 3)):
        part = vdr.pca.fit(x[sl], 3)
        assert_same_bits(part.components, whole.components[sl], ("components", sl))
        assert_same_bits(part.mean, whole.mean[sl], ("mean", sl))
        assert torch.equal(part.explained_variance, whole.explained_variance[sl])
        assert_same_bits(part.transform(x[sl], scale=True), whole.transform(x, scale=True)[sl], ("transform", sl))
