"""CPU: PCA of dense descriptors -- the four entry points are declared, bound and exported and refuse bad arguments before
they touch a device; the host-side refusals of vdr.ops.* / vdr.pca / pca_descriptors; the float64 restatement
(tests/pca_ref.py), composed on the CPU, against the golden files of sklearn and of the reference's own pca_colorize
(tests/golden/README_pca.md); the Otsu restatements agree with each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pca_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdr.h")
NAMES = ("vdr_pca_work_bytes", "vdr_op_col_mean", "vdr_op_covariance", "vdr_op_pca_project")


def test_header_binding_and_exports_declare_the_pca_entry_points():
    from vdr import _lib
    src = open(HDR).read()
    operand = r"const void\* x, int in_dtype, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,\s*"
    assert re.search(r"size_t vdr_pca_work_bytes\(int problems, int imgs, int t, int d\);", src)
    assert re.search(r"int vdr_op_col_mean\(" + operand + r"void\* work, float\* mean, void\* stream\);", src)
    assert re.search(r"int vdr_op_covariance\(" + operand + r"const float\* mean, void\* work, float\* cov, void\* stream\);", src)
    assert re.search(r"int vdr_op_pca_project\(" + operand + r"const float\* mean, const float\* comps, int k, int scale, void\* work, "
                     r"float\* proj, float\* minmax,\s*void\* stream\);", src)
    assert re.search(r"#define VDR_COV_CHUNK 1024\b", src)
    assert re.search(r"#define VDR_ABI_VERSION 8\b", src)
    declared = set(re.findall(r"\b(vdr_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert set(NAMES) <= declared and declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.vdr_abi_version() == 8
    import vdr
    from vdr import ops
    assert callable(ops.col_mean) and callable(ops.covariance) and callable(ops.pca_project)
    assert callable(vdr.pca.fit) and callable(vdr.pca_colorize) and callable(vdr.VitDescriptorModel.pca_descriptors)
    assert list(vdr.Pca.__dataclass_fields__) == ["mean", "components", "explained_variance", "explained_variance_ratio"]
    assert callable(vdr.Pca.transform)
    import inspect
    assert list(inspect.signature(vdr.VitDescriptorModel.pca_descriptors).parameters) == ["self", "x", "n_components", "layer", "facet",
                                                                                          "joint", "remove_bg"]
    assert list(inspect.signature(vdr.pca_colorize).parameters) == ["features", "output_shape", "remove_bg"]


def test_the_ops_refuse_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 16384)()
    base = (C.addressof(raw) + 255) & ~255
    X, WORK, MEAN, COV, COMPS, PROJ, MM = (base + 1024 * k for k in range(7))

    def mean(x=X, dt=1, ld=64, st=640, problems=2, imgs=1, t=10, d=64, work=WORK, mean=MEAN, **_):
        return lib.vdr_op_col_mean(x, dt, ld, st, problems, imgs, t, d, work, mean, None)

    def cov(x=X, dt=1, ld=64, st=640, problems=2, imgs=1, t=10, d=64, work=WORK, mean=MEAN, cov=COV, **_):
        return lib.vdr_op_covariance(x, dt, ld, st, problems, imgs, t, d, mean, work, cov, None)

    def proj(x=X, dt=1, ld=64, st=640, problems=2, imgs=1, t=10, d=64, work=WORK, mean=MEAN, comps=COMPS, k=3, scale=0, proj=PROJ,
             mm=MM, **_):
        return lib.vdr_op_pca_project(x, dt, ld, st, problems, imgs, t, d, mean, comps, k, scale, work, proj, mm, None)

    unsupported = [dict(d=16, ld=16), dict(d=48, ld=48), dict(d=33, ld=40), dict(d=2080, ld=2080), dict(d=4096, ld=4096)]
    invalid = [dict(x=None), dict(work=None), dict(mean=None), dict(problems=0), dict(problems=-1), dict(imgs=0), dict(t=0), dict(t=-3),
               dict(d=0), dict(d=-32), dict(ld=32), dict(ld=63), dict(st=-640), dict(dt=2), dict(dt=-1),
               dict(x=X + 2), dict(x=X + 8), dict(work=WORK + 4), dict(mean=MEAN + 8), dict(ld=68), dict(st=644),
               dict(dt=0, ld=66), dict(dt=0, st=642),
               dict(problems=2, t=2 ** 30), dict(problems=1, imgs=2 ** 16, t=2 ** 15), dict(problems=2 ** 11, imgs=2 ** 10, t=2 ** 10),
               dict(problems=2 ** 30, imgs=2 ** 30, t=2 ** 30), dict(problems=2 ** 31 - 1, imgs=2 ** 31 - 1, t=2 ** 31 - 1)]
    for op in (mean, cov, proj):
        for kw in unsupported:
            assert op(**kw) == -7, (op.__name__, kw)  # VDR_ERR_UNSUPPORTED
            assert b"d must be" in lib.vdr_last_error(None)
        for kw in invalid:
            assert op(**kw) == -1, (op.__name__, kw)  # VDR_ERR_INVALID
        # fp32 rows of 4 elements are 16-byte aligned; a stride of 0 is well formed: as far as the device check or the launch
        assert op(dt=0, ld=68, st=0) in (0, -2, -3)
    for kw in (dict(cov=None), dict(cov=COV + 4), dict(t=1), dict(imgs=1, t=1, problems=5)):
        assert cov(**kw) == -1, kw
    assert cov(imgs=2, t=1, st=64) in (0, -2, -3)  # (R = 2 rows over two images)
    for kw in (dict(comps=None), dict(proj=None), dict(mm=None), dict(comps=COMPS + 8), dict(proj=PROJ + 4), dict(mm=MM + 8)):
        assert proj(**kw) == -1, kw
    for k in (0, -1, 9, 64):
        assert proj(k=k) == -7, k
        assert b"k must be" in lib.vdr_last_error(None)
    assert proj(k=8) in (0, -2, -3) and proj(k=1, scale=1) in (0, -2, -3)


def test_work_bytes_covers_the_three_ops_and_is_aligned():
    from vdr import _lib
    wb = _lib.load().vdr_pca_work_bytes
    assert wb(0, 1, 1, 32) == 0 and wb(1, 1, 0, 32) == 0
    for problems, imgs, t, d in ((1, 1, 2, 32), (3, 1, 196, 768), (1, 64, 196, 768), (16, 1, 4096, 256), (1, 1, 3969, 768), (2, 3, 1025, 2048)):
        R, nt = imgs * t, -(-d // 128)
        chunks = -(-R // 1024)
        need = max(chunks * d, nt * (nt + 1) // 2 * chunks * 128 * 128, -(-R // 64) * 2) * problems * 4
        w = wb(problems, imgs, t, d)
        assert w % 16 == 0 and need <= w < need + 16, (problems, imgs, t, d, w, need)


def test_host_side_refusals_of_the_python_entry_points():
    import vdr
    from vdr import ops
    x = torch.zeros(2, 10, 64)
    for fn in (ops.col_mean, ops.covariance, lambda a: ops.pca_project(a, torch.zeros(2, 64), torch.zeros(2, 3, 64))):
        with pytest.raises(TypeError, match="HIP device"):
            fn(x)
        with pytest.raises(TypeError, match=r"\[P, t, d\]"):
            fn(torch.zeros(10, 64))
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            fn(x.double())
    with pytest.raises(ValueError, match="k must be 1..8"):
        ops.pca_project(x, torch.zeros(2, 64), torch.zeros(2, 9, 64))
    with pytest.raises(ValueError, match="sets of components"):
        ops.pca_project(x, torch.zeros(3, 64), torch.zeros(3, 3, 64))
    with pytest.raises(ValueError, match="n_components"):
        vdr.pca.fit(x, n_components=9)
    with pytest.raises(ValueError, match="n_components"):
        vdr.pca.fit(torch.zeros(1, 2, 64), n_components=3)
    with pytest.raises(ValueError, match="multiple of 32"):
        vdr.pca_colorize(np.zeros((16, 40), np.float32), (4, 4))
    with pytest.raises(ValueError, match="does not hold"):
        vdr.pca_colorize(np.zeros((16, 64), np.float32), (4, 5))
    # fewer rows than components: upstream's all-ones branch, no device needed
    for d in (64, 40):  # (upstream returns ones whatever the width)
        out = vdr.pca_colorize(np.zeros((2, d), np.float32), (1, 2))
        assert out.shape == (1, 2, 3) and out.dtype == np.float32 and np.all(out == 1.0)
    # pca_descriptors refuses a width the kernels do not take before it touches the engine (none is attached here)
    for dim in (2304, 80):
        m = object.__new__(vdr.VitDescriptorModel)
        m.cfg = vdr.VdrConfig(img=32, patch=8, dim=dim, heads=1, layers=1, mlp_hidden=64)
        with pytest.raises(ValueError, match="multiples of 32 up to 2048.*bin=True"):
            m.pca_descriptors(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("name", pref.SK_CASES)
def test_restatement_against_sklearn(golden_dir, name):
    g, x = pref.load_golden(golden_dir, name)
    assert np.all(g["eigen_ratios"] <= 0.6)
    mean, comps, lam, ratio = pref.fit(x, 3)
    cos = 1 - pref.component_cosine(comps.numpy(), g["components"])
    ev = np.abs(lam.numpy() - g["explained_variance"]) / g["explained_variance"]
    evr = np.abs(ratio.numpy() - g["explained_variance_ratio"]) / g["explained_variance_ratio"]
    rgb, _ = pref.colorize(x, (x.shape[0],))
    err, err_default = np.abs(rgb - g["rgb_full"]).max(), np.abs(rgb - g["rgb_default"]).max()
    print(name, "1-|cos|", cos.max(), "explained variance", ev.max(), "ratio", evr.max(), "rgb", err, "rgb (default solver)", err_default)
    assert np.all((comps.numpy() * g["components"]).sum(-1) > 0)  # the sign convention is sklearn's
    assert cos.max() <= pref.GATE_COS and ev.max() <= pref.GATE_EV and evr.max() <= pref.GATE_RATIO
    assert err <= pref.GATE_RGB and err_default <= pref.GATE_RGB


def test_restatement_against_the_references_pca_colorize(golden_dir):
    g, x = pref.load_golden(golden_dir, "pca_ref_colorize")
    assert np.all(g["eigen_ratios"] <= 0.6) and float(g["otsu_margin"]) > 1e-3
    rgb, _ = pref.colorize(x, (32, 32))
    rgb_bg, mask = pref.colorize(x, (32, 32), remove_bg=True)
    e0, e1 = np.abs(rgb - g["rgb"]).max(), np.abs(rgb_bg - g["rgb_remove_bg"]).max()
    print("pca_colorize", e0, "remove_bg", e1, "otsu", pref.otsu(rgb[..., 0]), float(g["otsu_threshold"]))
    assert np.array_equal(mask, g["mask"])
    assert e0 <= pref.GATE_REF_RGB and e1 <= pref.GATE_REF_RGB
    assert abs(pref.otsu(g["rgb"][..., 0]) - float(g["otsu_threshold"])) <= 1e-12  # the restated Otsu is skimage's on its own input


def test_the_librarys_otsu_and_remove_bg_are_the_restatement(golden_dir):
    """vdr.pca._otsu_threshold / remove_background are plain torch: they run on the host too"""
    from vdr import pca
    g = np.load(os.path.join(golden_dir, "pca_ref_colorize.npz"), allow_pickle=False)
    rgb = torch.from_numpy(g["rgb"])
    assert abs(float(pca._otsu_threshold(rgb[..., 0])) - float(g["otsu_threshold"])) <= 1e-12
    out = pca._remove_background(rgb)
    assert np.abs(out.numpy() - g["rgb_remove_bg"]).max() <= 1e-12
    gen = torch.Generator().manual_seed(0)
    for _ in range(3):
        a = torch.rand(37, 41, generator=gen) ** 2
        assert abs(float(pca._otsu_threshold(a)) - pref.otsu(a.numpy())) <= 1e-12
    assert float(pca._otsu_threshold(torch.full((4, 4), 0.25))) == 0.25
    const = torch.full((4, 4, 3), 0.5)
    assert torch.equal(pca._min_max_scale(const), const)
