"""CPU: the float64 restatement of vdr_op_mahalanobis (tests/mahalanobis_ref.py) fed scikit-learn's own parameters against
scikit-learn's recorded distances (tests/golden/anomaly_sk_*.npz, README_anomaly.md); an fp32 evaluation in another order
stays inside the restatement's bound; vdr.anomaly.whitening against numpy on the stored covariances; the accumulator's merge
against the covariance of the concatenation; the header and the binding agree, every C-ABI refusal of vdr_op_mahalanobis returns
its code before a device is touched, and without a GPU the op fails loudly; the host-side TypeErrors / ValueErrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mahalanobis_ref as mr
from fixtures import lib  # noqa: F401

GOLDENS = ("anomaly_sk_600x32", "anomaly_sk_1200x96", "anomaly_sk_1000x256")
POS = "anomaly_sk_pos_2x3x40x32"
SK_WORST = 1.44e-5  # README_anomaly.md: the worst relative distance of the restatement from sklearn's distances, measured here
SK_GATE = 4 * SK_WORST


def _untriu(v, d):
    a = np.zeros((d, d))
    a[np.triu_indices(d)] = v
    return a + np.triu(a, 1).T


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    c = np.load(os.path.join(golden_dir, name + "_cov.npz"))
    d = int(name.split("x")[-1])
    return z, {"emp": _untriu(c["emp_cov_triu"], d), "shr": _untriu(c["shr_cov_triu"], d)}


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_sklearn(golden_dir, name):
    z, cov = _load(golden_dir, name)
    assert z["train_bits"].dtype == np.uint16 and z["test_bits"].dtype == np.uint16
    for f in (name + ".npz", name + "_cov.npz"):
        assert os.path.getsize(os.path.join(golden_dir, f)) < 1000000
    test = mr.from_bf16_bits(z["test_bits"])
    out = z["is_outlier"]
    for tag in ("emp", "shr"):
        sk = z[tag + "_d2"]
        assert sk[out].min() >= 2.0 * sk[~out].max()  # (the generator's condition)
        w, vals = mr.whiten64(cov[tag])  # sklearn's own covariance_, whitened in float64, rounded once to fp32
        assert vals.min() > 0
        got = mr.d2(test, z["location"].astype(np.float32), w)
        rel = np.abs(got - sk) / sk
        print(f"{name} {tag}: restatement relative to sklearn, worst {rel.max():.3e}")
        assert rel.max() <= SK_GATE
        assert got[out].min() > got[~out].max()


def test_restatement_reproduces_sklearn_per_position(golden_dir):
    z = np.load(os.path.join(golden_dir, POS + ".npz"))
    test = mr.from_bf16_bits(z["test_bits"])
    gh, gw = z["grid"]
    assert test.shape[1] == gh * gw
    for p in range(test.shape[1]):
        w, _ = mr.whiten64(z["shr_cov"][p])
        got = mr.d2(test[:, p], z["location"][p].astype(np.float32), w)
        rel = np.abs(got - z["shr_d2"][:, p]) / z["shr_d2"][:, p]
        print(f"{POS} position {p}: restatement relative to sklearn, worst {rel.max():.3e}")
        assert rel.max() <= SK_GATE
    assert z["shr_d2"][z["is_outlier"]].min() >= 2.0 * z["shr_d2"][~z["is_outlier"]].max()


@pytest.mark.parametrize("shape", ((70, 9, 32), (50, 96, 96), (40, 130, 416)))
def test_an_fp32_evaluation_in_another_order_stays_inside_the_bound(shape):
    R, k, d = shape
    rng = np.random.default_rng(R + k + d)
    x = mr.bf16_rn(rng.normal(size=(R, d))).astype(np.float32)
    mean = (0.3 * rng.normal(size=d)).astype(np.float32)
    w = (rng.normal(size=(k, d)) / np.sqrt(d)).astype(np.float32)
    ref, bound = mr.d2(x, mean, w), mr.d2_bound(x, mean, w)
    zh, zl = (a.astype(np.float32) for a in mr.split(mr.centre(x, mean)))
    wh, wl = (a.astype(np.float32) for a in mr.split(w))
    # fp32 throughout, channels DESCENDING, the three products in separate accumulators, the squares summed descending
    acc = [np.zeros((R, k), np.float32) for _ in range(3)]
    for c in range(d - 1, -1, -1):
        for a, (p, q) in zip(acc, ((zh, wh), (zh, wl), (zl, wh))):
            a += p[:, c:c + 1] * q[:, c][None, :]
    yv = (acc[2] + acc[1]) + acc[0]
    got = np.zeros(R, np.float32)
    for j in range(k - 1, -1, -1):
        got = got + yv[:, j] * yv[:, j]
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    print(f"d = {d}, k = {k}: worst |d2_32 - d2_64| / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # what the definition leaves out: against the distance with the fp32 operands themselves
    full = (((x.astype(np.float64) - mean.astype(np.float64)) @ w.astype(np.float64).T) ** 2).sum(-1)
    assert (np.abs(ref - full) <= 1e-4 * full).all()


@pytest.mark.parametrize("name", GOLDENS[:2])
def test_whitening_against_numpy(golden_dir, name):
    from vdr import anomaly
    z, cov = _load(golden_dir, name)
    n = z["train_bits"].shape[0]
    d = cov["emp"].shape[0]
    s = torch.from_numpy(cov["emp"] * n / (n - 1)).unsqueeze(0)  # the n - 1 form that vdr.ops.covariance returns
    for shrinkage, ridge, nc in ((0.0, 0.0, None), (0.01, 0.0, None), (0.0, 0.01, 8), (0.3, 0.5, d)):
        w, vals = anomaly.whitening(s, n, shrinkage, ridge, nc)
        w64, v64 = mr.whiten64(cov["emp"], shrinkage, ridge, nc)
        k = d if nc is None else nc
        assert w.dtype == torch.float32 and tuple(w.shape) == (1, k, d) and vals.dtype == torch.float64
        assert np.allclose(vals[0].numpy(), v64, rtol=1e-10, atol=0)
        # rows are defined up to sign; W^T W = S^-1 restricted to the kept directions is not
        a, b = w[0].double().numpy(), w64
        assert np.allclose(a.T @ a, b.T @ b, rtol=0, atol=1e-5 * np.abs(b.T @ b).max())
        sign = np.sign((a * b).sum(-1))
        assert np.allclose(a * sign[:, None], b, rtol=0, atol=2e-6 * np.abs(b).max())
    shr = anomaly.whitening(s, n, 0.01)[0][0].double().numpy()
    assert np.allclose(shr.T @ shr, np.linalg.inv(cov["shr"]), rtol=0, atol=1e-5 * np.abs(np.linalg.inv(cov["shr"])).max())


def test_whitening_refusals():
    from vdr import anomaly
    eye = torch.eye(4, dtype=torch.float64).unsqueeze(0)
    singular = eye.clone()
    singular[0, 3, 3] = 0.0
    with pytest.raises(ValueError, match="shrinkage.*ridge"):
        anomaly.whitening(singular, 10)
    assert anomaly.whitening(singular, 10, shrinkage=0.1)[0].shape == (1, 4, 4)
    assert anomaly.whitening(singular, 10, ridge=0.01)[0].shape == (1, 4, 4)
    assert anomaly.whitening(singular, 10, n_components=3)[0].shape == (1, 3, 4)
    with pytest.raises(TypeError):
        anomaly.whitening(eye[0], 10)
    with pytest.raises(TypeError):
        anomaly.whitening(eye.to(torch.float16), 10)
    for kw in (dict(n=1), dict(n=10, shrinkage=-0.1), dict(n=10, shrinkage=1.5), dict(n=10, ridge=-1.0), dict(n=10, n_components=0),
               dict(n=10, n_components=5)):
        with pytest.raises(ValueError):
            anomaly.whitening(eye, **kw)


@pytest.mark.parametrize("per_position", (False, True))
def test_accumulator_merges_to_the_covariance_of_the_concatenation(per_position):
    from vdr import anomaly
    rng = np.random.default_rng(3)
    P, d = (5, 16) if per_position else (1, 16)
    batches = [rng.normal(size=(P, n, d)) + 100.0 * rng.normal(size=(P, 1, d)) for n in (7, 40, 2, 19)]
    acc = anomaly.GaussianAccumulator(per_position)
    for b in batches:
        m = b.mean(1)
        c = b - m[:, None, :]
        acc.merge(b.shape[1], torch.from_numpy(m), torch.from_numpy(np.einsum("pni,pnj->pij", c, c)))
    allrows = np.concatenate(batches, 1)
    assert acc.n == allrows.shape[1]
    want = np.stack([np.cov(allrows[p].T) for p in range(P)])
    assert np.allclose(acc.mean.numpy(), allrows.mean(1), rtol=0, atol=1e-12)
    assert np.allclose(acc.covariance().numpy(), want, rtol=0, atol=1e-9 * np.abs(want).max())
    g = acc.finish(shrinkage=0.01)
    assert g.n == acc.n and g.per_position == per_position and tuple(g.whiten.shape) == (P, d, d) and g.mean.dtype == torch.float32
    with pytest.raises(ValueError, match="no batch"):
        anomaly.GaussianAccumulator().finish()


def _aligned(n=4096):
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) & ~15


def _args(p, **kw):
    #        x, ld, image_stride, problem_stride, problems, imgs, t, d, mean, mean_stride, whiten, whiten_stride, k, d2, stream
    a = dict(x=p, ld=64, image_stride=640, problem_stride=1280, problems=2, imgs=2, t=10, d=64, mean=p, mean_stride=64, whiten=p,
             whiten_stride=192, k=3, d2=p, stream=None)
    a.update(kw)
    return list(a.values())


def test_header_and_binding_agree(lib):
    from vdr import _lib, ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdr.h")).read()
    m = re.search(r"int vdr_op_mahalanobis\(([^;]*)\);", hdr)
    params = [q.strip() for q in m.group(1).replace("\n", " ").split(",")]
    res, argtypes = _lib.SYMBOLS["vdr_op_mahalanobis"]
    assert res is C.c_int and len(params) == len(argtypes) == 15
    for q, t in zip(params, argtypes):
        want = C.c_void_p if "*" in q else C.c_int64 if q.startswith("int64_t") else C.c_int
        assert t is want, q
    assert hasattr(lib, "vdr_op_mahalanobis") and lib.vdr_abi_version() == 8
    assert int(re.search(r"#define VDR_MAHALANOBIS_MAX_K (\d+)", hdr).group(1)) == ops.MAHALANOBIS_MAX_K == 2048
    assert not hasattr(lib, "vdr_mahalanobis_work_bytes")  # the op needs no scratch


def test_op_refuses_bad_arguments_before_touching_a_device(lib):
    keep, p = _aligned()
    fn = lib.vdr_op_mahalanobis
    INVALID, UNSUPPORTED = -1, -7
    for name in ("x", "mean", "whiten", "d2"):
        assert fn(*_args(p, **{name: None})) == INVALID, name
        assert b"null" in lib.vdr_last_error(None)
    for name in ("x", "mean", "whiten"):
        assert fn(*_args(p, **{name: p + 4})) == INVALID, name  # misaligned
        assert b"aligned" in lib.vdr_last_error(None)
    assert fn(*_args(p, d2=p + 2)) == INVALID
    assert b"aligned" in lib.vdr_last_error(None)
    for name in ("problems", "imgs", "t", "d"):
        for v in (0, -1):
            assert fn(*_args(p, **{name: v})) == INVALID, (name, v)
    for d in (8, 48, 100):
        assert fn(*_args(p, d=d, ld=128)) == UNSUPPORTED, d
        assert b"multiple of 32" in lib.vdr_last_error(None)
    for k in (0, -3, 2049, 5000):
        assert fn(*_args(p, k=k, whiten_stride=0)) == UNSUPPORTED, k
        assert b"1..2048" in lib.vdr_last_error(None)
    assert fn(*_args(p, ld=56)) == INVALID  # ld < d
    for name in ("image_stride", "problem_stride"):
        assert fn(*_args(p, **{name: -8})) == INVALID, name
        assert fn(*_args(p, **{name: 12})) == INVALID, name  # not a multiple of 8 elements
        assert b"aligned" in lib.vdr_last_error(None)
    assert fn(*_args(p, ld=68)) == INVALID
    for name, low in (("mean_stride", 32), ("whiten_stride", 128)):
        assert fn(*_args(p, **{name: -4})) == INVALID, name
        assert fn(*_args(p, **{name: low})) == INVALID, name  # models overlap
        assert b"mean_stride" in lib.vdr_last_error(None)
    assert fn(*_args(p, mean_stride=66)) == INVALID and b"aligned" in lib.vdr_last_error(None)
    assert fn(*_args(p, whiten_stride=194)) == INVALID and b"aligned" in lib.vdr_last_error(None)
    assert fn(*_args(p, problems=2 ** 20, imgs=2 ** 6, t=2 ** 5)) == INVALID  # problems * R = 2^31
    assert b"2^31" in lib.vdr_last_error(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_gpu_means_loud_failure_not_fallback(lib):
    keep, p = _aligned()
    assert lib.vdr_op_mahalanobis(*_args(p)) == -2  # VDR_ERR_NO_DEVICE
    assert lib.vdr_op_mahalanobis(*_args(p, mean_stride=0, whiten_stride=0, problem_stride=0)) == -2  # (stride 0 is accepted)
    from vdr import anomaly, ops
    with pytest.raises(TypeError, match="HIP device"):
        ops.mahalanobis(torch.zeros(1, 4, 32), torch.zeros(1, 32), torch.zeros(1, 2, 32))
    g = anomaly.Gaussian(torch.zeros(1, 32), torch.zeros(1, 2, 32), torch.ones(1, 2, dtype=torch.float64), 10, False)
    with pytest.raises(TypeError, match="HIP device"):
        g.score(torch.zeros(1, 4, 32))


def test_host_side_refusals():
    import vdr
    from vdr import anomaly, ops
    assert vdr.anomaly is anomaly and vdr.Gaussian is anomaly.Gaussian and vdr.AnomalyMap is anomaly.AnomalyMap
    assert vdr.GaussianAccumulator is anomaly.GaussianAccumulator and vdr.MemoryBank is anomaly.MemoryBank
    assert vdr.fit_gaussian is anomaly.fit_gaussian
    with pytest.raises(TypeError):
        ops.mahalanobis("x", torch.zeros(1, 32), torch.zeros(1, 2, 32))
    with pytest.raises(TypeError):
        ops.mahalanobis(torch.zeros(4, 32), torch.zeros(1, 32), torch.zeros(1, 2, 32))
    with pytest.raises(TypeError):
        ops.mahalanobis(torch.zeros(1, 4, 32, dtype=torch.float16), torch.zeros(1, 32), torch.zeros(1, 2, 32))
    g = anomaly.Gaussian(torch.zeros(1, 32), torch.zeros(1, 2, 32), torch.ones(1, 2, dtype=torch.float64), 10, False)
    with pytest.raises(TypeError):
        g.score(torch.zeros(4, 32))
    with pytest.raises(ValueError, match="channels"):
        g.score(torch.zeros(1, 4, 64))
    gp = anomaly.Gaussian(torch.zeros(6, 32), torch.zeros(6, 2, 32), torch.ones(6, 2, dtype=torch.float64), 10, True, (2, 3))
    with pytest.raises(ValueError, match="positions"):
        gp.score(torch.zeros(2, 4, 32))
    with pytest.raises(TypeError):
        anomaly.GaussianAccumulator().add(torch.zeros(4, 32))
    with pytest.raises(ValueError, match="2 images"):
        anomaly.GaussianAccumulator(per_position=True).add(torch.zeros(1, 4, 32))
    with pytest.raises(TypeError):
        anomaly.MemoryBank(torch.zeros(3, 4, 32))
    with pytest.raises(TypeError):
        anomaly.MemoryBank(torch.zeros(4, 32)).score(torch.zeros(4, 32))
    with pytest.raises(ValueError):
        anomaly.MemoryBank.coreset(torch.zeros(2, 4, 32), 9)
    bank = anomaly.MemoryBank.coreset(torch.arange(8.0).view(1, 8, 1).expand(1, 8, 32).contiguous(), 2)
    assert bank.bank.dtype == torch.bfloat16 and bank.bank[:, 0].tolist() == [7.0, 0.0]  # maximin: largest norm, then farthest


def test_anomaly_map_on_hand_made_arrays():
    from vdr import anomaly
    d2 = torch.zeros(2, 4, 4)
    d2[0, 1, 2], d2[1, 3, 0] = 9.0, 4.0
    m = anomaly.AnomalyMap(d2)
    assert m.score.tolist() == [9.0, 4.0]
    up = m.upsample((16, 16))
    assert tuple(up.shape) == (2, 16, 16)
    assert torch.equal(up, torch.nn.functional.interpolate(d2.unsqueeze(1), size=(16, 16), mode="bilinear", align_corners=False)[:, 0])
    blur = m.upsample((16, 16), sigma=2.0)
    assert tuple(blur.shape) == (2, 16, 16) and float(blur.max()) < float(up.max())
    assert torch.allclose(blur.sum((1, 2)), anomaly.gaussian_blur(up, 2.0).sum((1, 2)))
    flat = torch.full((1, 8, 8), 3.0)
    assert torch.allclose(anomaly.gaussian_blur(flat, 1.5), flat, atol=1e-6)  # (the weights sum to one, borders replicated)
    assert anomaly.gaussian_blur(flat, 0.0) is flat
