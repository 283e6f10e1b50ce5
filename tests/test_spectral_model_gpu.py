"""GPU: vdr.spectral on the device ops, and VitDescriptorModel.tokencut / lost on the tiny network of
tests/test_correspondences_gpu.py (image 32, patch 8, D = 64, 2 blocks: a 4 x 4 grid; 7 x 7 at patch stride 4).

On the goldens (tests/golden/README_spectral.md) the graph of the kernel must be the stored float64 graph word for word (no
score lies within 4 x bound of tau), and fiedler on it is held to SciPy's dense eigen-decomposition.  The two gates are
10 x the values measured on an MI355X with this code (MEASURED below: the first run, written down before any gate existed;
README_spectral.md and DESIGN 4.6n carry the same figures), the margin being for device-to-device differences in torch's
float64 reductions.  Labels: TokenCut's bipartition against the golden's, rows with
|f_i - mean| <= 1e-3 max|f - mean| left out (none on these maps)."""
import numpy as np
import pytest
import torch

import handle_configs as hc
import spectral_ref as sref
from handle_configs import TINY
from oracle import vit_oracle as vo
from spectral_ref import NAMES, labels_agree, load_golden

pytestmark = pytest.mark.gpu


# name: (|lambda - golden|, 1 - |cos|) as first measured on the device
MEASURED = {"130x32": (1.063e-08, 9.548e-15), "333x96": (3.743e-09, 7.772e-16), "520x416": (1.540e-08, 9.659e-15)}


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_spectral_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return vo.make_images(TINY, 3, seed=6).cuda()


@pytest.mark.parametrize("name", NAMES)
def test_goldens_graph_eigenpair_and_labels(name):
    from vdr import ops, spectral
    g, t, b, x = load_golden(name)
    bits = ops.affinity_bits(x[None].cuda(), tau=float(g["tau"]))
    assert np.array_equal(bits.cpu().numpy(), sref.pack(b[None])), name
    deg = spectral.degree(bits)
    assert deg.dtype == torch.int32 and np.array_equal(deg.cpu().numpy()[0], b.sum(1))
    vec, val, resid, steps = spectral.fiedler(bits, eps=float(g["eps"]))
    dl = abs(float(val[0]) - g["eigvals"][1])
    dc = 1.0 - abs(float(vec[0].cpu().numpy() @ g["fiedler"]))
    ml, mc = MEASURED[name]
    print(f"{name}: steps {steps}, |lambda - golden| {dl:.3e} (measured {ml:.3e}), 1 - |cos| {dc:.3e} (measured {mc:.3e}), "
          f"residual estimate {float(resid[0]):.3e}")
    assert float(resid[0]) <= 1e-6 and steps <= 32
    assert dl <= 10 * ml
    assert dc <= 10 * mc
    labels_agree(vec[0].cpu().numpy(), g, name)
    res = spectral.tokencut(bits, tuple(g["grid"]), eps=float(g["eps"]))
    rp, rs, rm, rb = sref.tokencut(res.eigvec[0].cpu().numpy(), tuple(g["grid"]))
    assert np.array_equal(res.bipartition[0].cpu().numpy(), rp) and int(res.seed[0]) == rs
    assert np.array_equal(res.mask[0].cpu().numpy(), rm) and tuple(res.box[0].tolist()) == rb
    assert torch.equal(res.eigvec.reshape(1, -1), vec)  # deterministic: the second run is the first


def test_lost_on_a_golden_graph_follows_the_reference_rule():
    from vdr import ops, spectral
    g, t, _, x = load_golden("333x96")
    bits = ops.affinity_bits(x[None].cuda().expand(2, -1, -1), tau=0.0)
    s0 = sref.similarity(x[None])
    b0 = ops.unpack_bits(bits, t)[1].cpu().numpy()  # the device's graph; it is the float64 one outside the band of the bound
    clear = np.abs(s0[0]) > sref.bound(x[None], s0)[0]
    assert clear.mean() > 0.99 and np.array_equal(b0[clear], (s0[0] > 0)[clear]) and np.array_equal(b0, b0.T)
    grid = tuple(g["grid"])
    for k in (1, 40, 100, 1000):
        res = spectral.lost(bits, grid, k=k, stride=4, patch=8)
        seed, chosen, mask, box = sref.lost(b0, grid, k)
        for p in range(2):
            assert int(res.seed[p]) == seed and np.array_equal(res.expansion[p].cpu().numpy(), chosen)
            assert np.array_equal(res.mask[p].cpu().numpy(), mask) and tuple(res.box[p].tolist()) == box
        assert res.degree.dtype == torch.int32 and np.array_equal(res.degree.reshape(2, -1)[0].cpu().numpy(), b0.sum(1))
        assert torch.equal(res.pixel_box(), res.box.float() * 4 + 4.0) and res.bits is bits


def _median_cosine(desc):
    """the median cosine between the rows of desc [B, t, d]: a threshold at which the graph has both kinds of entries (the tiny
    random network's descriptors share a large common component: every cosine is above 0.5, so the graph at tau = 0.2 -- and
    at LOST's tau = 0 -- is complete and says nothing about tau, facet or layer)"""
    dn = torch.nn.functional.normalize(desc.double(), dim=-1)
    return float(torch.quantile((dn @ dn.transpose(1, 2)).flatten(), 0.5))


def _edge_shares(ops, bits, t):
    return ops.unpack_bits(bits, t).double().mean(dim=(1, 2))


@pytest.mark.parametrize("setup", ((8, 32), (4, 32), (8, 48)), ids=("default", "stride4", "size48"))
def test_model_tokencut_and_lost(model, images, setup):
    import vdr
    from vdr import ops, spectral
    stride, side = setup
    x = images
    if side != 32:
        x = torch.nn.functional.interpolate(x, size=(side, side), mode="bilinear", align_corners=False)
        model.set_input_size(side, side)
    model.set_patch_stride(stride)
    try:
        gs = (side - 8) // stride + 1
        t = gs * gs
        # extract_descriptors' output rounded to bf16 is what the forward writes for the bf16 facet
        desc = model.extract_descriptors(x)[:, 0].to(torch.bfloat16)
        tau = _median_cosine(desc)
        tc = model.tokencut(x, tau=tau)
        assert isinstance(tc, vdr.TokenCut) and tc.grid == (gs, gs) and tc.stride == stride and tc.patch == 8
        assert tuple(tc.eigvec.shape) == (3, gs, gs) and tc.eigvec.dtype == torch.float64
        assert tuple(tc.bipartition.shape) == (3, gs, gs) and tc.bipartition.dtype == torch.bool
        assert tuple(tc.mask.shape) == (3, gs, gs) and tuple(tc.box.shape) == (3, 4) and tuple(tc.seed.shape) == (3,)
        assert torch.isfinite(tc.eigvec).all() and torch.isfinite(tc.eigval).all() and 1 <= tc.steps <= 32
        # the graph itself, word for word, and it is a graph with both kinds of entries in every image
        bits = ops.affinity_bits(desc, tau=tau)
        assert torch.equal(tc.bits, bits)
        shares = _edge_shares(ops, bits, t)
        print(f"{setup}: tau {tau:.4f}, edge shares {[round(float(v), 3) for v in shares]}, eigval {[round(float(v), 4) for v in tc.eigval]}")
        assert bool(((shares > 0.1) & (shares < 0.9)).all())
        for other in (dict(tau=tau + 0.05), dict(tau=tau, facet="query"), dict(tau=tau, layer=0)):  # each of them shows in the bits
            assert not torch.equal(model.tokencut(x, **other).bits, bits), other
        want = spectral.tokencut(bits, (gs, gs), stride=stride, patch=8)
        for f in ("eigvec", "bipartition", "seed", "mask", "box", "eigval"):
            assert torch.equal(getattr(tc, f), getattr(want, f)), f
        for p in range(3):  # the rules, on the returned eigenvector
            rp, rs, rm, rb = sref.tokencut(tc.eigvec[p].cpu().numpy(), (gs, gs))
            assert np.array_equal(tc.bipartition[p].cpu().numpy(), rp) and int(tc.seed[p]) == rs
            assert np.array_equal(tc.mask[p].cpu().numpy(), rm) and tuple(tc.box[p].tolist()) == rb
            assert bool(tc.mask[p].reshape(-1)[rs])
        again = model.tokencut(x, tau=tau)
        for f in ("eigvec", "bipartition", "seed", "mask", "box", "eigval", "bits"):
            assert torch.equal(getattr(tc, f), getattr(again, f)), f
        assert torch.equal(model.tokencut(x).bits, ops.affinity_bits(desc, tau=0.2))  # the default threshold
        # lost: the default graph is the one at tau = 0 (complete on this network); the rule is checked at the median
        k = max(2, t // 3)
        assert torch.equal(model.lost(x, k=k).bits, ops.affinity_bits(desc, tau=0.0))
        lo = model.lost(x, k=k, tau=tau)
        assert isinstance(lo, vdr.Lost) and tuple(lo.mask.shape) == (3, gs, gs) and lo.grid == (gs, gs)
        assert torch.equal(lo.bits, bits)
        b0 = ops.unpack_bits(bits, t).cpu().numpy()
        for p in range(3):
            seed, chosen, mask, box = sref.lost(b0[p], (gs, gs), k)
            assert int(lo.seed[p]) == seed and np.array_equal(lo.expansion[p].cpu().numpy(), chosen)
            assert np.array_equal(lo.mask[p].cpu().numpy(), mask) and tuple(lo.box[p].tolist()) == box
            assert np.array_equal(lo.degree[p].cpu().numpy().reshape(-1), b0[p].sum(1))
        lo2 = model.lost(x, k=k, tau=tau)
        assert torch.equal(lo.mask, lo2.mask) and torch.equal(lo.box, lo2.box)
    finally:
        model.set_patch_stride(8)
        if side != 32:
            model.set_input_size(32, 32)


def test_model_dynamic_size_other_facets_and_refusals(model, images):
    import vdr
    name = "_spectral_tiny_dyn"
    vdr.ARCHS[name] = hc.vit_config(TINY)
    try:
        dyn = vdr.load_model(name, weights=vo.make_weights(TINY, seed=21, scale=0.05), dynamic_size=True)
    finally:
        del vdr.ARCHS[name]
    x48 = torch.nn.functional.interpolate(images, size=(48, 40), mode="bilinear", align_corners=False)
    tc = dyn.tokencut(x48)
    assert tc.grid == (6, 5) and tuple(tc.mask.shape) == (3, 6, 5)
    assert tuple(dyn.lost(images, k=5).mask.shape) == (3, 4, 4)
    fixed = model.tokencut(images, tau=0.8)  # (about the median cosine of this network's keys: a graph with both kinds of entries)
    back = dyn.tokencut(images, tau=0.8)
    share = float(vdr.ops.unpack_bits(fixed.bits, 16).double().mean())
    assert 0.1 < share < 0.9, share
    assert torch.equal(fixed.bits, back.bits) and torch.equal(fixed.eigvec, back.eigvec) and torch.equal(fixed.mask, back.mask)
    assert tuple(model.tokencut(images, layer=0, facet="token", bin=True).eigvec.shape) == (3, 4, 4)
    assert tuple(model.lost(images, layer=0, facet="value", k=3).box.shape) == (3, 4)
    for call in (lambda: model.tokencut(images, facet="nope"), lambda: model.tokencut(images, layer=99),
                 lambda: model.tokencut(images, bin=True, hierarchy=5), lambda: model.tokencut(images[0]),
                 lambda: model.lost(images, k=0), lambda: model.lost(images, k=2.5), lambda: model.lost(images, facet="nope"),
                 lambda: model.tokencut(images, tau=float("nan")), lambda: model.lost(images, tau=float("nan"))):
        with pytest.raises(ValueError):
            call()
