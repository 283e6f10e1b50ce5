"""CPU: the Gram side and the top-k solver of the PCA -- the five entry points are declared, bound and exported and refuse
bad arguments before they touch a device; the host-side refusals and the side choice of vdr.pca.fit(solver="subspace");
the float64 restatement of the subspace iteration (tests/pca_topk_ref.py) against numpy.linalg.eigh on planted spectra; on
the golden sklearn maps the Gram route of the restatement gives the components of the covariance route."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pca_ref as pref
import pca_topk_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")
NAMES = ("vdr_pca_topk_work_bytes", "vdr_op_col_mean_any", "vdr_op_gram", "vdr_op_pca_back_project", "vdr_op_sym_topk")
from vdr import ops as _ops  # noqa: E402

TOL, MAX_ITER = _ops.TOPK_TOL, _ops.TOPK_MAX_ITER


def test_header_binding_and_exports_declare_the_entry_points():
    from vdr import _lib, ops
    src = open(HDR).read()
    operand = r"const void\* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int t, int d,\s*"
    assert re.search(r"size_t vdr_pca_topk_work_bytes\(int problems, int t, int d, int k\);", src)
    assert re.search(r"int vdr_op_col_mean_any\(" + operand + r"void\* work,\s*float\* mean, void\* stream\);", src)
    assert re.search(r"int vdr_op_gram\(" + operand + r"const float\* mean,\s*void\* work, float\* gram, void\* stream\);", src)
    assert re.search(r"int vdr_op_pca_back_project\(" + operand + r"const float\* mean, const float\* u, const float\* values, int k, "
                     r"void\* work, float\* comps,\s*void\* stream\);", src)
    assert re.search(r"int vdr_op_sym_topk\(const float\* a, int problems, int n, int k, float tol, int max_iter, void\* work, "
                     r"float\* values,\s*float\* vectors, int32_t\* iters, float\* resid, void\* stream\);", src)
    assert re.search(r"#define VDR_ABI_VERSION 8\b", src)
    assert int(re.search(r"#define VDR_GRAM_CHUNK (\d+)\b", src).group(1)) == tref.GRAM_CHUNK
    assert int(re.search(r"#define VDR_TOPK_SLAB (\d+)\b", src).group(1)) == tref.TOPK_SLAB
    assert float(re.search(r"#define VDR_TOPK_TOL ([0-9.e-]+)f", src).group(1)) == ops.TOPK_TOL
    assert int(re.search(r"#define VDR_TOPK_MAX_ITER (\d+)\b", src).group(1)) == ops.TOPK_MAX_ITER
    lib = _lib.load()
    assert all(n in _lib.SYMBOLS and hasattr(lib, n) for n in NAMES) and lib.vdr_abi_version() == 8
    import inspect
    import vdr
    assert all(callable(getattr(ops, n)) for n in ("col_mean_any", "gram", "sym_topk", "pca_back_project"))
    assert list(inspect.signature(vdr.pca.fit).parameters)[:4] == ["x", "n_components", "joint", "solver"]
    assert inspect.signature(vdr.pca.fit).parameters["solver"].default == "eigh"
    assert inspect.signature(vdr.pca.colorize).parameters["solver"].default == "eigh"
    sig = inspect.signature(vdr.VitDescriptorModel.pca_descriptor_maps).parameters
    assert (sig["bin"].default, sig["hierarchy"].default, sig["solver"].default) == (False, 2, "eigh")
    assert issubclass(vdr.pca.ConvergenceWarning, Warning)


def test_work_bytes_covers_the_ops():
    from vdr import _lib
    wb = _lib.load().vdr_pca_topk_work_bytes
    assert wb(0, 4, 32, 1) == 0 and wb(1, 0, 32, 1) == 0
    for P, t, d, k in ((1, 2, 32, 1), (3, 196, 768, 3), (1, 196, 13056, 3), (2, 729, 13056, 8), (1, 4096, 256, 8), (4, 300, 288, 3)):
        nt, chunks = -(-t // 128), -(-d // tref.GRAM_CHUNK)
        mean = -(-t // 1024) * d
        gram = nt * (nt + 1) // 2 * chunks * 128 * 128
        back = -(-t // 1024) * k * d
        nslab = -(-t // tref.TOPK_SLAB)
        need = max(max(mean, gram, back) * P * 4, ((3 + nslab) * t * 16 * P + P) * 4)  # solver: V, W, Z, slab partials, flags
        w = wb(P, t, d, k)
        assert w % 16 == 0 and need <= w < need + 32, (P, t, d, k, w, need)


def test_the_ops_refuse_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 16384)()
    base = (C.addressof(raw) + 255) & ~255
    X, WORK, MEAN, OUT, U, VAL, IT, RES = (base + 1024 * k for k in range(8))

    def mean(x=X, dt=1, ld=64, st=640, problems=2, t=10, d=64, work=WORK, mean=MEAN, **_):
        return lib.vdr_op_col_mean_any(x, dt, ld, st, problems, t, d, work, mean, None)

    def gram(x=X, dt=1, ld=64, st=640, problems=2, t=10, d=64, work=WORK, mean=MEAN, out=OUT, **_):
        return lib.vdr_op_gram(x, dt, ld, st, problems, t, d, mean, work, out, None)

    def back(x=X, dt=1, ld=64, st=640, problems=2, t=10, d=64, work=WORK, mean=MEAN, out=OUT, u=U, val=VAL, k=3, **_):
        return lib.vdr_op_pca_back_project(x, dt, ld, st, problems, t, d, mean, u, val, k, work, out, None)

    def topk(a=X, problems=2, n=10, k=3, tol=1e-5, max_iter=4, work=WORK, val=VAL, vec=OUT, it=IT, res=RES):
        return lib.vdr_op_sym_topk(a, problems, n, k, tol, max_iter, work, val, vec, it, res, None)

    invalid = [dict(x=None), dict(work=None), dict(mean=None), dict(problems=0), dict(t=0), dict(t=-3), dict(d=0), dict(d=-32),
               dict(ld=32), dict(st=-640), dict(dt=2), dict(x=X + 8), dict(work=WORK + 4), dict(mean=MEAN + 8), dict(ld=68),
               dict(st=644), dict(dt=0, ld=66), dict(problems=2 ** 20, t=2 ** 12)]
    for op in (mean, gram, back):
        for kw in (dict(d=16, ld=16), dict(d=48, ld=48), dict(d=33, ld=40)):
            assert op(**kw) == -7, (op.__name__, kw)  # VDR_ERR_UNSUPPORTED
            assert b"d must be" in lib.vdr_last_error(None)
        for kw in invalid:
            assert op(**kw) == -1, (op.__name__, kw)  # VDR_ERR_INVALID
        if not torch.cuda.is_available():  # (with a GPU present an accepted call would launch on these dummy host buffers)
            assert op(d=4096, ld=4096) in (-2, -3) and op(d=13056, ld=13056) in (-2, -3)  # no upper bound on d
    for t in (1, 4097):
        assert gram(t=t) == -7 and b"t must be" in lib.vdr_last_error(None)
    assert gram(out=None) == -1 and gram(out=OUT + 4) == -1
    for kw in (dict(u=None), dict(val=None), dict(out=None), dict(u=U + 8)):
        assert back(**kw) == -1, kw
    for k in (0, 9):
        assert back(k=k) == -7
    for kw in (dict(n=1), dict(n=4097), dict(k=0), dict(k=9), dict(n=2, k=3)):
        assert topk(**kw) == -7, kw
    for kw in (dict(a=None), dict(work=None), dict(val=None), dict(vec=None), dict(it=None), dict(res=None), dict(problems=0),
               dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=0), dict(a=X + 4), dict(work=WORK + 8)):
        assert topk(**kw) == -1, kw
    if not torch.cuda.is_available():
        assert topk() in (-2, -3) and topk(n=2, k=2, tol=0.0) in (-2, -3)


def test_host_side_refusals_of_the_python_entry_points():
    import vdr
    from vdr import ops
    x = torch.zeros(2, 10, 64)
    for fn in (ops.col_mean_any, ops.gram, lambda a: ops.pca_back_project(a, torch.zeros(2, 64), torch.zeros(2, 3, 10), torch.zeros(2, 3))):
        with pytest.raises(TypeError, match="HIP device"):
            fn(x)
        with pytest.raises(TypeError, match=r"\[P, t, d\]"):
            fn(torch.zeros(10, 64))
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            fn(x.double())
    with pytest.raises(TypeError, match="HIP device"):
        ops.sym_topk(torch.zeros(1, 8, 8), 3)
    with pytest.raises(TypeError, match=r"\[P, n, n\]"):
        ops.sym_topk(torch.zeros(1, 8, 9), 3)
    with pytest.raises(ValueError, match="k must be 1..8"):
        ops.pca_back_project(x, torch.zeros(2, 64), torch.zeros(2, 9, 10), torch.zeros(2, 9))
    # fit(solver="subspace"): all before any device work (the tensors live on the host)
    with pytest.raises(ValueError, match="solver must be one of"):
        vdr.pca.fit(x, solver="lanczos")
    with pytest.raises(ValueError, match="rows - 1"):
        vdr.pca.fit(torch.zeros(1, 3, 64), n_components=3, solver="subspace")
    with pytest.raises(ValueError, match="joint PCA takes the covariance side"):
        vdr.pca.fit(torch.zeros(2, 10, 2304), joint=True, solver="subspace")
    with pytest.raises(ValueError, match="t <= 4096"):
        vdr.pca.fit(torch.zeros(1, 4097, 13056), solver="subspace")
    with pytest.raises(ValueError, match="multiple of 32"):
        vdr.pca.fit(torch.zeros(1, 10, 40), solver="subspace")
    with pytest.raises(ValueError, match="covariance side takes d <= 2048"):
        vdr.pca.fit(torch.zeros(1, 10, 4096), solver="subspace", side="covariance")
    with pytest.raises(ValueError, match="multiple of 32"):
        vdr.pca.colorize(np.zeros((16, 40), np.float32), (4, 4), solver="subspace")
    with pytest.raises(ValueError, match="at most 2048"):
        vdr.pca.colorize(np.zeros((16, 4096), np.float32), (4, 4))  # the default solver keeps its limit
    out = vdr.pca.colorize(np.zeros((2, 4096), np.float32), (1, 2), solver="subspace")
    assert out.shape == (1, 2, 3) and np.all(out == 1.0)
    # Pca.transform stops at the projection kernel's width, and says so
    p = vdr.Pca(torch.zeros(1, 4096), torch.zeros(1, 3, 4096), torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="stops at d = 2048.*scores"):
        p.transform(torch.zeros(1, 10, 4096))
    # the model: a default call on a wide model still raises the old message; the new keywords are checked device-free
    m = object.__new__(vdr.VitDescriptorModel)
    m.cfg = vdr.VdrConfig(img=32, patch=8, dim=2304, heads=1, layers=1, mlp_hidden=64)
    with pytest.raises(ValueError, match="multiples of 32 up to 2048.*bin=True"):
        m.pca_descriptors(torch.zeros(1, 3, 32, 32))
    m.cfg = vdr.VdrConfig(img=32, patch=8, dim=256, heads=1, layers=1, mlp_hidden=64)
    with pytest.raises(ValueError, match="multiples of 32 up to 2048.*bin=True"):
        m.pca_descriptor_maps(torch.zeros(1, 3, 32, 32), facet="key", bin=True)  # 17 * 256 channels, default solver
    with pytest.raises(ValueError, match="bin needs a facet"):
        m.pca_descriptor_maps(torch.zeros(1, 3, 32, 32), bin=True, solver="subspace")
    with pytest.raises(ValueError, match="solver must be one of"):
        m.pca_descriptor_maps(torch.zeros(1, 3, 32, 32), solver="svd")
    with pytest.raises(ValueError, match="hierarchy must be"):
        m.pca_descriptor_maps(torch.zeros(1, 3, 32, 32), facet="key", bin=True, hierarchy=4, solver="subspace")


def test_the_side_choice_of_the_subspace_solver():
    from vdr import pca
    assert pca.subspace_side(1, 196, 768, False) == "gram"
    assert pca.subspace_side(16, 196, 768, False) == "gram"       # per image: rows = 196 < 768
    assert pca.subspace_side(16, 196, 768, True) == "covariance"  # joint, whatever the row count
    assert pca.subspace_side(2, 196, 768, True) == "covariance"
    assert pca.subspace_side(1, 1024, 256, False) == "covariance"
    assert pca.subspace_side(1, 768, 768, False) == "covariance"  # rows >= d
    assert pca.subspace_side(1, 767, 768, False) == "gram"
    assert pca.subspace_side(1, 196, 13056, False) == "gram"
    assert pca.subspace_side(1, 3969, 2304, False) == "gram"      # rows >= d, but beyond the covariance kernel's width
    assert pca.subspace_side(1, 2048, 2048, False) == "covariance"
    assert pca._check_subspace(1, 3969, 768, 3, False) == "covariance" and pca._check_subspace(1, 729, 13056, 3, False) == "gram"


def test_the_start_block_is_the_stated_hash_and_has_full_rank():
    # two entries worked out by hand from the definition in include/vdr.h
    def h(r, c):
        m = 0xFFFFFFFF
        x = ((r * 0x9E3779B1) & m) ^ ((c * 0x85EBCA6B) & m)
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & m
        x ^= x >> 12
        x = (x * 0x297A2D39) & m
        x ^= x >> 15
        return -1.0 if x & 1 else 1.0
    pat = tref.start_hash(300, 16)
    assert all(pat[r, c] == h(r, c) for r, c in ((0, 0), (1, 0), (0, 1), (17, 5), (299, 15), (128, 8)))
    assert abs(pat.mean()) < 0.1  # (both signs occur about equally often)
    for n in list(range(17, 65)) + [127, 200, 768, 4096]:
        assert np.linalg.matrix_rank(tref.start_hash(n, 16)) == 16, n
        v = tref.orthonormalise(tref.start_block(n))
        assert np.abs(v.T @ v - np.eye(16)).max() < 1e-6, n
    assert np.array_equal(tref.orthonormalise(tref.start_block(5))[:, :5], np.eye(5))


def test_the_round_robin_jacobi_diagonalises():
    rng = np.random.default_rng(0)
    for scale in (1.0, 1e-6):
        a = rng.standard_normal((16, 16)) * np.logspace(0, -8, 16)
        a = (a @ a.T) * scale
        theta, y = tref.jacobi16(a)
        w = np.linalg.eigvalsh(a)
        assert np.abs(np.sort(theta) - w).max() <= 1e-14 * w[-1]
        assert np.abs(y.T @ y - np.eye(16)).max() <= 1e-14
        assert np.abs(y.T @ a @ y - np.diag(theta)).max() <= 1e-14 * w[-1]
    assert sorted(tuple(sorted((i, tref.partner(i, s)))) for s in range(15) for i in range(16) if i < tref.partner(i, s)) == \
        [(i, j) for i in range(16) for j in range(i + 1, 16)]  # every pair once per sweep


@pytest.mark.parametrize("n", (2, 15, 16, 17, 33, 200))
@pytest.mark.parametrize("ratio", (0.5, 0.9))
def test_restated_subspace_iteration_against_numpy_eigh(n, ratio):
    a, q, lam = tref.planted(n, tref.geometric(n, ratio), seed=n)
    w, v = np.linalg.eigh(a.astype(np.float64))
    w, v = w[::-1], v[:, ::-1]
    for k in (1, 3, 8):
        if k > n:
            continue
        val, vec, iters, resid = tref.sym_topk(a, k, TOL, MAX_ITER)
        assert resid <= TOL and iters < MAX_ITER
        vec = vec.astype(np.float64)
        # the contract: float64 residual <= tol * lambda_1, plus the fp32 rounding of the returned pair
        res = np.linalg.norm(a.astype(np.float64) @ vec.T - vec.T * val.astype(np.float64), axis=0)
        assert res.max() <= (TOL + 4 * pref.U) * w[0], (k, res.max())
        assert np.abs(val - w[:k]).max() <= (TOL + 2 * pref.U) * w[0]  # |theta - lambda| <= ||residual||, one fp32 rounding
        assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() <= 4 * pref.U
        for j in range(k):  # Davis-Kahan: sin(angle) <= residual / gap
            gap = np.abs(np.delete(w, j) - val[j]).min()
            sin = tref.sine(vec[j], v[:, j])
            assert sin <= res[j] / gap + 4 * pref.U * np.sqrt(n), (k, j, sin, res[j] / gap)
            at = int(np.argmax(np.abs(vec[j])))
            assert vec[j, at] > 0


def test_restated_solver_reports_a_flat_tail_and_solves_rank_two():
    lam = np.concatenate([[1.0, 0.5], 0.25 * 0.9999 ** np.arange(62)])
    a, _, _ = tref.planted(64, lam, seed=6)
    _, _, iters, resid = tref.sym_topk(a, 3, TOL, MAX_ITER)
    assert iters == MAX_ITER and resid > TOL
    lam = np.zeros(40)
    lam[:2] = (3.0, 1.0)
    a, q, _ = tref.planted(40, lam, seed=5)
    val, vec, iters, resid = tref.sym_topk(a, 2, TOL, MAX_ITER)
    assert resid <= TOL and iters <= 3 and np.abs(val - (3.0, 1.0)).max() <= 1e-6
    assert np.abs(np.abs((vec.astype(np.float64) * q[:, :2].T).sum(1)) - 1).max() <= 1e-6


@pytest.mark.parametrize("name", pref.SK_CASES)
def test_gram_route_of_the_restatement_gives_the_covariance_routes_components(golden_dir, name):
    g, x = pref.load_golden(golden_dir, name)
    t, d = x.shape
    mean, comps_c, lam_c, ratio_c, _ = tref.fit(x, 3, "covariance", TOL, MAX_ITER)
    _, comps_g, lam_g, ratio_g, scores = tref.fit(x, 3, "gram", TOL, MAX_ITER)
    cos = 1 - pref.component_cosine(comps_c.numpy(), comps_g.numpy())
    ev = np.abs(lam_c.numpy() - lam_g.numpy()) / lam_c.numpy()
    print(name, "1-|cos|", cos.max(), "explained variance", ev.max())
    # both routes decompose z^T z and z z^T of the same bf16-centred z: same spectrum, components related by z^T u
    assert cos.max() <= pref.GATE_COS and ev.max() <= pref.GATE_EV
    assert np.all((comps_c.numpy() * comps_g.numpy()).sum(-1) > 0)  # one sign rule
    # and both meet the gates the eigh route is held to against sklearn
    for comps, lam, ratio in ((comps_c, lam_c, ratio_c), (comps_g, lam_g, ratio_g)):
        assert (1 - pref.component_cosine(comps.numpy(), g["components"])).max() <= pref.GATE_COS
        assert (np.abs(lam.numpy() - g["explained_variance"]) / g["explained_variance"]).max() <= pref.GATE_EV
        assert (np.abs(ratio.numpy() - g["explained_variance_ratio"]) / g["explained_variance_ratio"]).max() <= pref.GATE_RATIO
    # the scores are the projection of the map on the components
    proj = pref.project(x, mean, comps_g)[0].numpy()
    # (the Gram matrix is built from the bf16-rounded centred map, the projection from the fp32 one: 2^-9 per entry)
    assert np.abs(scores - proj).max() <= 2.0 ** -8 * np.abs(proj).max()
