"""GPU: VitDescriptorModel.pca_descriptor_maps -- pca_descriptors with the log-binning of extract_descriptors and the
solver of vdr.pca.fit as keywords -- on the tiny network of tests/test_pca_model_gpu.py (image 32, patch 8, D = 64, 2 blocks).

With solver="subspace" a log-binned key facet (17 x 64 = 1088 channels on 16, 49 or 30 patches: the Gram side) must be, bit
for bit, vdr.pca.colorize(solver="subspace") of the rows extract_descriptors(bin=True) returns, at the default grid, at patch
stride 4 and at another input size.  Without binning both solvers must colour a map alike, to the gate the eigh route is
held to against sklearn."""
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
    with hc.registered_model("_pca_topk_tiny") as m:
        yield m


def test_binned_pca_descriptors_is_colorize_of_the_binned_rows(model):
    import vdr
    x = vo.make_images(TINY, 3, seed=6).cuda()
    gh, gw = 4, 4
    for hierarchy in (2, 1):
        rows = model.extract_descriptors(x, facet="key", bin=True, hierarchy=hierarchy)[:, 0]
        d = (1 + 8 * hierarchy) * TINY.dim
        assert rows.shape == (3, gh * gw, d) and vdr.pca.subspace_side(1, gh * gw, d, False) == "gram"
        got = model.pca_descriptor_maps(x, facet="key", bin=True, hierarchy=hierarchy, solver="subspace")
        assert got.shape == (3, gh, gw, 3) and got.dtype == torch.float32 and float(got.min()) == 0.0 and float(got.max()) == 1.0
        for b in range(3):
            assert_same_bits(got[b], vdr.pca.colorize(rows[b].to(torch.bfloat16), (gh, gw), solver="subspace"), ("per image", hierarchy, b))
        bg = model.pca_descriptor_maps(x, facet="key", bin=True, hierarchy=hierarchy, remove_bg=True, solver="subspace")
        assert_same_bits(bg[1], vdr.pca.colorize(rows[1].to(torch.bfloat16), (gh, gw), remove_bg=True, solver="subspace"), ("remove_bg", hierarchy))


def test_binned_pca_descriptors_follows_the_patch_stride_and_the_input_size(model):
    import vdr
    x = vo.make_images(TINY, 2, seed=7).cuda()

    def check(x, grid):
        gh, gw = grid
        assert tuple(model.grid) == grid
        rows = model.extract_descriptors(x, facet="key", bin=True)[:, 0]
        got = model.pca_descriptor_maps(x, facet="key", bin=True, solver="subspace")
        assert got.shape == (2, gh, gw, 3)
        for b in range(2):
            assert_same_bits(got[b], vdr.pca.colorize(rows[b].to(torch.bfloat16), (gh, gw), solver="subspace"), (grid, b))

    model.set_patch_stride(4)
    try:
        check(x, (7, 7))
    finally:
        model.set_patch_stride(8)
    big = torch.nn.functional.interpolate(x, size=(48, 40), mode="bilinear", align_corners=False)
    model.set_input_size(48, 40)
    try:
        check(big, (6, 5))
    finally:
        model.set_input_size(32, 32)


def test_the_default_solver_still_refuses_wide_binned_descriptors():
    """at D = 256 a binned facet has 17 x 256 = 4352 channels: refused by default, coloured with solver="subspace" """
    import vdr
    cfg = vo.VitCfg(32, 8, 3, 256, 2, 1, 256)
    vdr.ARCHS["_pca_topk_wide"] = hc.vit_config(cfg)
    try:
        m = vdr.load_model("_pca_topk_wide", weights=vo.make_weights(cfg, seed=3, scale=0.05))
    finally:
        del vdr.ARCHS["_pca_topk_wide"]
    x = vo.make_images(cfg, 2, seed=1).cuda()
    with pytest.raises(ValueError, match="multiples of 32 up to 2048.*bin=True"):
        m.pca_descriptor_maps(x, facet="key", bin=True)
    with pytest.raises(ValueError, match="joint PCA takes the covariance side"):
        m.pca_descriptor_maps(x, facet="key", bin=True, joint=True, solver="subspace")
    got = m.pca_descriptor_maps(x, facet="key", bin=True, solver="subspace")
    rows = m.extract_descriptors(x, facet="key", bin=True)[:, 0]
    assert rows.shape == (2, 16, 4352) and got.shape == (2, 4, 4, 3)
    for b in range(2):
        assert_same_bits(got[b], vdr.pca.colorize(rows[b].to(torch.bfloat16), (4, 4), solver="subspace"), ("wide", b))
    with pytest.raises(ValueError, match="at most 2048"):
        vdr.pca_colorize(rows[0], (4, 4))


def test_both_solvers_colour_an_unbinned_map_alike(model):
    x = vo.make_images(TINY, 3, seed=6).cuda()
    model.set_patch_stride(2)  # 13 x 13 = 169 patches of 64 channels: the covariance side
    try:
        for kw in ({}, dict(facet="key"), dict(joint=True)):
            a = model.pca_descriptors(x, **kw)
            b = model.pca_descriptor_maps(x, solver="subspace", **kw)
            assert_same_bits(model.pca_descriptor_maps(x, **kw), a, ("the defaults are pca_descriptors", kw))
            err = float((a - b).abs().max())
            print("eigh against subspace", kw, err)
            assert a.shape == b.shape == (3, 13, 13, 3) and err <= pref.GATE_RGB, (kw, err)
    finally:
        model.set_patch_stride(8)
    # 16 patches of 64 channels: the Gram side
    a = model.pca_descriptors(x, facet="key")
    b = model.pca_descriptor_maps(x, facet="key", solver="subspace")
    err = float((a - b).abs().max())
    print("eigh against subspace (Gram side)", err)
    assert err <= pref.GATE_RGB
