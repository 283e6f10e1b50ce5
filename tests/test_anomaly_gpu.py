"""GPU: vdr.anomaly on the device against scikit-learn's recorded fits (tests/golden/anomaly_sk_*.npz, README_anomaly.md) and
VitDescriptorModel.fit_anomaly / anomaly_map on the tiny network of tests/test_correspondences_gpu.py (image 32, patch 8,
D = 64, 2 blocks: a 4 x 4 grid; 7 x 7 at patch stride 4).

Every golden map goes through fit_gaussian + score -- the library's own mean, covariance and whitening.  The distance to
scikit-learn is dominated by vdr.ops.covariance's one bf16 rounding of the centred rows in the FIT (2^-9 per entry, amplified
along the small-variance directions); it cannot be derived, so it is measured: FIT_WORST is the first value measured on an
MI355X, the gate ten times that (the margin of README_spectral.md); the per-position case has its own pair.  Independently of the gate every planted outlier must
score above every inlier (the generator made sklearn's own margin a factor 2 at least)."""
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
from handle_configs import TINY
import mahalanobis_ref as mr
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

GOLDENS = ("anomaly_sk_600x32", "anomaly_sk_1200x96", "anomaly_sk_1000x256")
POS = "anomaly_sk_pos_2x3x40x32"
FIT_WORST = 1.57e-3  # README_anomaly.md: the worst relative distance of fit_gaussian + score from sklearn's distances over the
FIT_GATE = 10 * FIT_WORST  # three global maps, first device run (anomaly_sk_1000x256, empirical covariance)
POS_WORST = 9.36e-3  # the same of the per-position case: 40 rows per Gaussian of 32 channels, a fit ten times as ill-conditioned
POS_GATE = 10 * POS_WORST


@pytest.fixture(scope="module")
def anomaly():
    from vdr import anomaly
    return anomaly


def _bf16(bits):
    return torch.from_numpy(mr.from_bf16_bits(bits)).cuda().to(torch.bfloat16)


@pytest.mark.parametrize("name", GOLDENS)
def test_fit_and_score_reproduce_sklearn(anomaly, golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    train, test, out = _bf16(z["train_bits"]).unsqueeze(0), _bf16(z["test_bits"]).unsqueeze(0), z["is_outlier"]
    n, d = train.shape[1:]
    for tag, shrinkage in (("emp", 0.0), ("shr", float(z["shrinkage"]))):
        g = anomaly.fit_gaussian(train, shrinkage=shrinkage)
        assert g.n == n and not g.per_position and tuple(g.mean.shape) == (1, d) and tuple(g.whiten.shape) == (1, d, d)
        assert np.abs(g.mean[0].cpu().numpy().astype(np.float64) - z["location"]).max() <= 1e-5
        got = g.score(test)
        assert tuple(got.shape) == (1, test.shape[1]) and got.dtype == torch.float32
        got = got[0].cpu().numpy().astype(np.float64)
        sk = z[tag + "_d2"]
        rel = np.abs(got - sk) / sk
        print(f"{name} {tag}: fit_gaussian + score relative to sklearn, worst {rel.max():.3e}")
        assert rel.max() <= FIT_GATE
        assert got[out].min() > got[~out].max()
        # the score IS the op on the fitted model, and the op stays inside the restatement's bound of that model
        ref = mr.d2(test[0].float().cpu().numpy(), g.mean[0].cpu().numpy(), g.whiten[0].cpu().numpy())
        assert (np.abs(got - ref) <= mr.d2_bound(test[0].float().cpu().numpy(), g.mean[0].cpu().numpy(), g.whiten[0].cpu().numpy())).all()
    few = anomaly.fit_gaussian(train, shrinkage=0.01, n_components=8)
    assert tuple(few.whiten.shape) == (1, 8, d) and bool((few.score(test) <= g.score(test) * (1 + 1e-5)).all())


def test_per_position_fit_and_score_reproduce_sklearn(anomaly, golden_dir):
    z = np.load(os.path.join(golden_dir, POS + ".npz"))
    train, test, out = _bf16(z["train_bits"]), _bf16(z["test_bits"]), z["is_outlier"]
    imgs, t, d = train.shape
    g = anomaly.fit_gaussian(train, per_position=True, shrinkage=float(z["shrinkage"]))
    assert g.per_position and g.n == imgs and tuple(g.mean.shape) == (t, d) and tuple(g.whiten.shape) == (t, d, d)
    got = g.score(test)
    assert tuple(got.shape) == tuple(test.shape[:2]) and got.is_contiguous()
    got = got.cpu().numpy().astype(np.float64)
    rel = np.abs(got - z["shr_d2"]) / z["shr_d2"]
    print(f"{POS}: fit_gaussian + score relative to sklearn, worst {rel.max():.3e}")
    assert rel.max() <= POS_GATE
    assert got[out].min() > got[~out].max()
    # position p is problem p: the same bits as a global model of position p alone
    for p in (0, t - 1):
        one = anomaly.Gaussian(g.mean[p:p + 1], g.whiten[p:p + 1], g.eigenvalues[p:p + 1], g.n, False)
        assert torch.equal(one.score(test[:, p:p + 1].contiguous())[:, 0], g.score(test)[:, p])
    # fp32 rows and a view take the same route
    assert torch.equal(g.score(test.float()), g.score(test))
    wide = torch.full((test.shape[0], t, 3 * d), float("nan"), dtype=torch.bfloat16).cuda()
    wide[:, :, d:2 * d] = test
    assert torch.equal(g.score(wide[:, :, d:2 * d]), g.score(test))
    with pytest.raises(ValueError, match="positions"):
        g.score(test[:, :t - 1])


@pytest.mark.parametrize("per_position", (False, True))
def test_accumulator_over_batches_equals_the_one_batch_fit(anomaly, golden_dir, per_position):
    """Both fits round the centred rows once to bf16 -- around the batch's mean and around the overall mean -- so each covariance
    entry is within 2^-8 (1 + 2^-9) sqrt(c_ii c_jj) of the exact one (|dz| <= 2^-9 |z| on either factor, Cauchy-Schwarz over the
    rows); the float64 merge itself and the fp32 sums of the kernels add terms four orders below that.  The two fits therefore
    differ by at most 2^-7 sqrt(c_ii c_jj), taken with 1 % of slack."""
    z = np.load(os.path.join(golden_dir, POS + ".npz"))
    x = _bf16(z["train_bits"])  # [40, 6, 32]
    one = anomaly.GaussianAccumulator(per_position).add(x)
    acc = anomaly.GaussianAccumulator(per_position)
    for lo, hi in ((0, 7), (7, 30), (30, 40)):
        acc.add(x[lo:hi])
    assert acc.n == one.n == (40 if per_position else 240)
    assert torch.allclose(acc.mean, one.mean, rtol=0, atol=1e-5)
    c1, c3 = one.covariance(), acc.covariance()
    dg = c1.diagonal(dim1=1, dim2=2)
    bound = 1.01 * 2.0 ** -7 * (dg.unsqueeze(2) * dg.unsqueeze(1)).sqrt()
    print(f"per_position {per_position}: worst |cov_3 - cov_1| / bound {float(((c3 - c1).abs() / bound).max()):.3f}")
    assert bool(((c3 - c1).abs() <= bound).all())
    assert not torch.equal(c3, c1)
    g1, g3 = one.finish(shrinkage=0.01), acc.finish(shrinkage=0.01)
    test = _bf16(z["test_bits"])
    assert torch.allclose(g3.score(test), g1.score(test), rtol=0.05)
    with pytest.raises(ValueError, match="after batches"):
        acc.add(torch.zeros((40, 6, 64), dtype=torch.bfloat16).cuda())


def test_memory_bank(anomaly):
    from vdr import kmeans, ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((3, 50, 64), generator=gen).cuda().to(torch.bfloat16)
    bank = anomaly.MemoryBank.coreset(x, 20)
    rows = x.reshape(1, 150, 64)
    idx = kmeans.maximin(rows, 20)[0]
    assert torch.equal(bank.bank, rows[0][idx]) and bank.bank.dtype == torch.bfloat16
    got = bank.score(x)
    sim = ops.nn_cosine(x, bank.bank.unsqueeze(0).expand(3, 20, 64), mutual=False)[0]
    assert tuple(got.shape) == (3, 50) and torch.equal(got, 1.0 - sim)
    assert bool((got.reshape(-1)[idx] <= 1e-6).all())  # a bank row is at distance 0 from itself
    assert torch.equal(anomaly.MemoryBank(rows[0][idx].float()).score(x), got)


@pytest.fixture(scope="module")
def model():
    with hc.registered_model("_anomaly_tiny") as m:
        yield m


@pytest.fixture(scope="module")
def images():
    return [vo.make_images(TINY, 3, seed=s).cuda() for s in (6, 9, 12)]


@pytest.mark.parametrize("per_position", (False, True))
@pytest.mark.parametrize("stride", (8, 4))
def test_anomaly_map_is_the_composition_of_its_pieces(anomaly, model, images, stride, per_position):
    model.set_patch_stride(stride)
    try:
        g = (32 - 8) // stride + 1
        gauss = model.fit_anomaly(images[:2], per_position=per_position)
        assert isinstance(gauss, anomaly.Gaussian) and gauss.grid == (g, g) and gauss.per_position == per_position
        assert gauss.n == (6 if per_position else 6 * g * g) and tuple(gauss.whiten.shape) == (g * g if per_position else 1, 64, 64)
        amap = model.anomaly_map(images[2], gauss)
        assert isinstance(amap, anomaly.AnomalyMap) and tuple(amap.d2.shape) == (3, g, g) and amap.d2.dtype == torch.float32
        desc = model.extract_descriptors(images[2])[:, 0]  # [B, t, d] fp32
        assert torch.equal(amap.d2.reshape(3, -1), gauss.score(desc))
        assert torch.equal(amap.score, amap.d2.reshape(3, -1).max(dim=1).values)
        assert tuple(amap.upsample((32, 32), sigma=1.0).shape) == (3, 32, 32)
        # the fit is the accumulator over the same descriptors
        acc = anomaly.GaussianAccumulator(per_position)
        for x in images[:2]:
            acc.add(model.extract_descriptors(x)[:, 0].to(torch.bfloat16))
        want = acc.finish(shrinkage=0.01)
        assert torch.equal(want.mean, gauss.mean) and torch.equal(want.whiten, gauss.whiten)
    finally:
        model.set_patch_stride(8)


def test_model_refusals(anomaly, model, images):
    gauss = model.fit_anomaly(images[:2], per_position=True, layer=0, facet="value")
    assert gauss.grid == (4, 4)
    assert tuple(model.anomaly_map(images[2], gauss, layer=0, facet="value").d2.shape) == (3, 4, 4)
    model.set_patch_stride(4)
    try:
        with pytest.raises(ValueError, match="grid"):
            model.anomaly_map(images[2], gauss)
    finally:
        model.set_patch_stride(8)
    glob = model.fit_anomaly(images[:1], n_components=16)
    assert tuple(glob.whiten.shape) == (1, 16, 64)
    model.set_patch_stride(4)
    try:
        assert tuple(model.anomaly_map(images[2], glob).d2.shape) == (3, 7, 7)  # (a global model goes with any grid)
    finally:
        model.set_patch_stride(8)
    binned = model.fit_anomaly(images[:2], bin=True, hierarchy=1, shrinkage=0.1)
    assert tuple(binned.mean.shape) == (1, 9 * 64)
    with pytest.raises(ValueError, match="channels"):
        model.anomaly_map(images[2], binned)
    with pytest.raises(TypeError):
        model.anomaly_map(images[2], "gaussian")
    with pytest.raises(ValueError):
        model.fit_anomaly(images[:1], facet="keys")
    with pytest.raises(ValueError):
        model.anomaly_map(images[2], glob, layer=7)
    with pytest.raises(ValueError, match="B, 3, H, W"):
        model.anomaly_map(images[2][0], glob)
    with pytest.raises(ValueError, match="shrinkage.*ridge"):
        model.fit_anomaly(images[:1], shrinkage=0.0)  # 16 rows, 64 channels: singular


def test_fit_refuses_more_than_2048_channels(anomaly):
    import vdr
    wide = vo.VitCfg(32, 8, 3, 128, 2, 1, 256)  # binned at hierarchy 2: 17 * 128 = 2176 channels
    name = "_anomaly_wide"
    vdr.ARCHS[name] = hc.vit_config(wide)
    try:
        m = vdr.load_model(name, weights=vo.make_weights(wide, seed=3, scale=0.05))
        x = vo.make_images(wide, 2, seed=1).cuda()
        with pytest.raises(ValueError, match="at most 2048"):
            m.fit_anomaly([x], bin=True, hierarchy=2)
        g = m.fit_anomaly([x], bin=True, hierarchy=1, shrinkage=0.1, n_components=8)  # 9 * 128 = 1152 channels pass
        assert tuple(g.whiten.shape) == (1, 8, 1152) and tuple(m.anomaly_map(x, g, bin=True, hierarchy=1).d2.shape) == (2, 4, 4)
    finally:
        del vdr.ARCHS[name]
