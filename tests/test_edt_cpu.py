"""CPU: Euclidean distance transforms without a device -- the torch statement vdr.morphology.edt_torch against
scipy.ndimage.distance_transform_edt, the goldens it wrote (tests/golden/README_edt.md) and brute force (d2, the lowest-index rule
of `nearest`, the `outside` rule against a padded plane, the peak); the reference helpers of tests/edt_ref.py against each other;
dilation, erosion and the boundary against scipy's binary morphology with the Euclidean disc; the surface measures against their
restatement on scipy; the host program over csrc/edt_map.h, which runs the kernels' own passes thread by thread in both orders,
plainly and under the sanitizers; the symbols; every refusal of the C entry point before the device is touched; the refusals of
the Python layers.  Every output of the op is an integer: the gate is equality."""
import ctypes as C
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

import edt_ref as ER
import host_program

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")
NONE = ER.NONE


def _golden(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "edt_sp_*.npz")))
    assert len(files) == 6
    for f in files:
        z = np.load(f)
        H, W = (int(v) for v in z["shape"])
        yield os.path.basename(f), z, np.unpackbits(z["mask"])[:H * W].reshape(H, W)


def _unpack(z, key, shape):
    return np.unpackbits(z[key])[:shape[0] * shape[1]].reshape(shape)


SMALL = [(1, 1), (1, 7), (6, 1), (2, 2), (5, 9), (17, 16), (24, 19), (16, 24)]


def _small_planes(H, W):
    out = ER.planes(H, W)
    out["bernoulli0.8"] = ER.bernoulli(H, W, 0.8, H + W)
    return out


# ---- the statement, scipy, brute force and the goldens ------------------------------------------------------------------------------
def test_torch_statement_equals_the_goldens_scipy_wrote(golden_dir):
    from vdr import morphology as mo
    for name, z, m in _golden(golden_dir):
        t = torch.from_numpy(m)
        for value in (0, 1):
            for outside in (0, 1):
                d2 = mo.edt_torch(t, value, bool(outside))
                assert d2.dtype == torch.int32 and tuple(d2.shape) == m.shape
                assert np.array_equal(d2.numpy(), z[f"d2_v{value}_o{outside}"]), (name, value, outside)
        assert np.array_equal(mo.dilate(t, 3.5).numpy(), _unpack(z, "dilate", m.shape)), name
        assert np.array_equal(mo.erode(t.bool(), 3.5).numpy(), _unpack(z, "erode", m.shape).astype(bool)), name


@pytest.mark.parametrize("H,W", SMALL)
def test_torch_statement_equals_scipy_and_brute_force_on_small_planes(H, W):
    """d2 in the four modes; nearest attains d2 and is the lowest such index; the peak; `outside` is the plane padded by one
    non-selected pixel; the helpers of edt_ref agree with each other"""
    from vdr import morphology as mo
    for name, m in _small_planes(H, W).items():
        t = torch.from_numpy(m)
        for value in (0, 1):
            bd, bn = ER.brute(m, value)
            assert np.array_equal(ER.scipy_d2(m, value), bd), (name, value)
            assert np.array_equal(ER.nearest_given_d2(m, bd, value), bn), (name, value)
            d2, nearest, peak = mo.edt_torch(t, value, return_nearest=True, return_peak=True)
            assert np.array_equal(d2.numpy(), bd) and np.array_equal(nearest.numpy(), bn), (name, value)
            assert nearest.dtype == peak.dtype == torch.int32 and peak.tolist() == [list(ER.peak(bd))], (name, value)
            sel = ER.selected(m, value)
            if (~sel).any():                                               # the nearest pixel is not selected and is d2 away
                ny, nx = np.divmod(bn[sel], W)
                yy, xx = np.nonzero(sel)
                assert not sel[ny, nx].any() and np.array_equal((yy - ny) ** 2 + (xx - nx) ** 2, bd[sel])
            od = ER.brute(m, value, outside=True)[0]
            assert np.array_equal(ER.scipy_d2(m, value, outside=True), od), (name, value)
            d2o, peako = mo.edt_torch(t, value, outside=True, return_peak=True)
            assert np.array_equal(d2o.numpy(), od) and peako.tolist() == [list(ER.peak(od))], (name, value)
    full = torch.ones((H, W), dtype=torch.uint8)
    assert bool((mo.edt_torch(full) == NONE).all()) and np.array_equal(mo.edt_torch(full, outside=True).numpy(), ER.closed_form_outside_full(H, W))
    assert mo.edt_torch(full, return_peak=True)[1].tolist() == [[NONE, 0]] and mo.edt_torch(1 - full, return_peak=True)[1].tolist() == [[0, -1]]


def test_torch_statement_on_a_batch_and_on_the_long_planes():
    from vdr import morphology as mo
    pl = ER.planes(21, 70)
    stack = torch.from_numpy(np.stack(list(pl.values())))
    d2, nearest, peak = mo.edt_torch(stack, return_nearest=True, return_peak=True)
    for k, (name, m) in enumerate(pl.items()):
        bd, bn = ER.brute(m)
        assert np.array_equal(d2[k].numpy(), bd) and np.array_equal(nearest[k].numpy(), bn) and peak[k].tolist() == list(ER.peak(bd)), name
    for shape in ((1, 4096), (4096, 1)):                                    # the 16-bit row distance and the search depth at their limits
        m = np.ones(shape, np.uint8)
        m[0, 0] = 0
        d2 = mo.edt_torch(torch.from_numpy(m)).numpy().reshape(-1)
        assert np.array_equal(d2, np.arange(4096, dtype=np.int64) ** 2) and d2.max() == 4095 ** 2


# ---- morphology, boundary, points -----------------------------------------------------------------------------------------------------
def test_morphology_equals_scipy_with_the_disc():
    from scipy import ndimage
    from vdr import morphology as mo
    rng = np.random.default_rng(5)
    planes = [ER.bernoulli(37, 53, p, 9) for p in (0.02, 0.5, 0.97)] + [np.zeros((37, 53), np.uint8), np.ones((37, 53), np.uint8)]
    coarse = ndimage.zoom(rng.standard_normal((7, 9)), 8, order=1)[:37, :53]
    planes.append((coarse > 0.2).astype(np.uint8))
    for m in planes:
        t = torch.from_numpy(m)
        for r in (0, 0.5, 1, 1.5, 2, 2.9, 3.5, 7):
            want_d = ndimage.binary_dilation(m != 0, ER.disc(r)) if r >= 1 else m != 0
            want_e = ndimage.binary_erosion(m != 0, ER.disc(r)) if r >= 1 else m != 0
            want_in = ndimage.binary_erosion(m != 0, ER.disc(r), border_value=1) if r >= 1 else m != 0
            assert np.array_equal(mo.dilate(t, r).numpy() != 0, want_d), r
            assert np.array_equal(mo.erode(t, r).numpy() != 0, want_e), r
            assert np.array_equal(mo.erode(t, r, outside=False).numpy() != 0, want_in), r
            assert np.array_equal(mo.opening(t, r).numpy() != 0, ndimage.binary_dilation(want_e, ER.disc(r)) if r >= 1 else m != 0), r
            assert np.array_equal(mo.closing(t, r, outside=True).numpy() != 0, ndimage.binary_erosion(want_d, ER.disc(r)) if r >= 1 else m != 0), r
            assert np.array_equal(mo.closing(t, r).numpy() != 0, ndimage.binary_erosion(want_d, ER.disc(r), border_value=1) if r >= 1 else m != 0), r
        assert mo.dilate(t, 0) is t and mo.erode(t, 0.99) is t and mo.dilate(t.bool(), 2).dtype == torch.bool and mo.dilate(t, 2).dtype == torch.uint8
        assert np.array_equal(mo.boundary(t).numpy() != 0, (m != 0) ^ ndimage.binary_erosion(m != 0, ER.CROSS))
        ring = mo.ring(t, 1.5, 4).numpy() != 0
        assert np.array_equal(ring, ndimage.binary_dilation(m != 0, ER.disc(4)) & ~ndimage.binary_dilation(m != 0, ER.disc(1.5)))
        assert np.array_equal(mo.ring(t, 0, 3).numpy() != 0, ndimage.binary_dilation(m != 0, ER.disc(3)) & ~(m != 0))
        sd = mo.signed_distance(t)
        assert sd.dtype == torch.float32
        if 0 < m.sum() < m.size:
            want = np.where(m != 0, ndimage.distance_transform_edt(m != 0), -ndimage.distance_transform_edt(m == 0))
            assert np.array_equal(sd.numpy(), want.astype(np.float32))
    assert bool(torch.isposinf(mo.signed_distance(torch.ones((3, 3), dtype=torch.bool))).all())
    assert bool(torch.isneginf(mo.signed_distance(torch.zeros((3, 3), dtype=torch.bool))).all())


def test_inner_point_is_the_peak_in_prompt_coordinates():
    from vdr import morphology as mo
    m = torch.zeros((3, 16, 16), dtype=torch.bool)
    m[0, 2:9, 3:10] = True                                                  # a 7 x 7 square: the centre (5, 6), d2 = 16
    m[1, 0:4, 0:16] = True                                                  # a band on the edge: rows 1 and 2 tie, the lowest index wins
    pts, lab = mo.inner_point(m)
    assert pts.dtype == torch.float32 and lab.dtype == torch.int32 and lab.tolist() == [1, 1, -1]
    assert pts.tolist() == [[6.0, 5.0], [1.0, 1.0], [0.0, 0.0]]
    assert mo.inner_point(m, outside=False)[0][1].tolist() == [0.0, 0.0]     # without the outside the band's far edge is most interior
    pts, _ = mo.inner_point(m, 64)
    s = np.float32(64) / np.float32(16)
    assert pts[0].tolist() == [float((np.float32(6) + np.float32(0.5)) * s - np.float32(0.5)), float((np.float32(5) + np.float32(0.5)) * s - np.float32(0.5))]
    assert mo.inner_point(m[0], (32, 64))[0].tolist() == [[25.5, 10.5]]
    d2 = mo.edt_torch(m, outside=True)
    for p in range(2):
        x, y = (int(v) for v in mo.inner_point(m)[0][p].tolist())
        assert bool(m[p, y, x]) and int(d2[p, y, x]) == int(d2[p].max())


# ---- the measures -----------------------------------------------------------------------------------------------------------------------
def test_metrics_equal_their_scipy_restatement():
    """hd bitwise at spacing 1 (the same sqrt of the same integer); the float64 means and percentiles, and spacing != 1 against
    scipy's `sampling`, at rtol 1e-12: a few float64 roundings (2^-53 each) with three orders of margin -- derived, not measured"""
    from scipy import ndimage
    from vdr import metrics
    rng = np.random.default_rng(3)
    masks = []
    for seed in range(6):
        coarse = ndimage.zoom(np.random.default_rng(seed).standard_normal((6, 8)), 8, order=1)[:41, :57]
        masks.append(coarse > 0.1 * seed)
    masks += [np.zeros((41, 57), bool), rng.random((41, 57)) < 0.5]
    a, b = np.stack(masks), np.stack(masks[1:] + masks[:1])
    a[7], b[7] = False, False                                               # two empty masks
    ov = metrics.overlap(torch.from_numpy(a), torch.from_numpy(b))
    for k in range(len(a)):
        inter, na, nb = int((a[k] & b[k]).sum()), int(a[k].sum()), int(b[k].sum())
        assert [int(ov[n][k]) for n in ("intersection", "a", "b")] == [inter, na, nb]
        assert float(ov["dice"][k]) == (2.0 * inter / (na + nb) if na + nb else 1.0) and float(ov["iou"][k]) == (inter / (na + nb - inter) if na + nb else 1.0)
    for spacing, tol in ((1.0, 1.0), (1.0, 2.5), (0.7, 1.5)):
        got = metrics.surface(torch.from_numpy(a), torch.from_numpy(b), spacing=spacing, tolerance=tol)
        for k in range(len(a)):
            want = ER.surface_scipy(a[k], b[k], spacing, tol)
            for name in ("hd", "hd95", "assd", "nsd"):
                g, w = float(got[name][k]), want[name]
                if spacing == 1.0 and name == "hd":
                    assert g == w, (k, name)
                assert g == w or abs(g - w) <= 1e-12 * abs(w), (k, name, spacing, g, w)
    empty = metrics.surface(torch.from_numpy(a[:1]), torch.zeros((1, 41, 57), dtype=torch.bool))
    assert [float(empty[n][0]) for n in ("hd", "hd95", "assd", "nsd")] == [float("inf")] * 3 + [0.0]
    both = metrics.surface(torch.zeros((41, 57), dtype=torch.bool), torch.zeros((41, 57), dtype=torch.bool))
    assert [float(both[n][0]) for n in ("hd", "hd95", "assd", "nsd")] == [0.0, 0.0, 0.0, 1.0]
    for bad in (dict(spacing=0), dict(spacing=float("nan")), dict(tolerance=-1)):
        with pytest.raises(ValueError, match="surface"):
            metrics.surface(torch.from_numpy(a), torch.from_numpy(b), **bad)
    with pytest.raises(ValueError, match="overlap"):
        metrics.overlap(torch.from_numpy(a), torch.from_numpy(b[:, :40]))


# ---- the host program ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_kernels_passes_run_on_the_host_in_both_orders(tmp_path, sanitize):
    """tests/edt_map_cases.cpp, a host program with its own main, over the header the kernels include: each pass owns every pixel
    once, every index stays inside the promised extents, and the passes themselves, run thread by thread forward and reversed
    with every search under its step cap, give the brute-force d2, nearest and peak; the second build runs it under the address
    and undefined-behaviour sanitizers (host code, stand-alone)"""
    out = host_program.run("edt_map_cases", tmp_path, sanitize)
    lines = out.splitlines()
    assert lines[-1] == "cases 57 fails 0" and "FAIL" not in out
    assert sum(ln.endswith(" fails 0") and ln.startswith("H ") for ln in lines) == 57
    assert any(ln.startswith("H 300 W 517: seg 9 pitch 10 rblocks 75 ctiles 171 ") for ln in lines)
    assert any(ln.startswith("H 1 W 4096: seg 64 pitch 66 rblocks 1 ctiles 64 ") for ln in lines) and any(ln.startswith("H 4096 W 1: seg 1 pitch 2 ") for ln in lines)


# ---- the C side ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_listed_in_the_makefile():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint vdr_op_distance_transform\(", src) and "vdr_op_distance_transform" in _lib.SYMBOLS and hasattr(lib, "vdr_op_distance_transform")
    assert re.search(r"\bsize_t vdr_distance_transform_workspace_bytes\(", src) and hasattr(lib, "vdr_distance_transform_workspace_bytes")
    assert lib.vdr_abi_version() == 8 and "#define VDR_ABI_VERSION 8" in src               # additive: the version stays
    assert "#define VDR_EDT_NONE 2147483647" in src and "#define VDR_EDT_MAX_SIDE 4096" in src and "the lower x, across rows the lowest y'" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^NOCONTRACT :=.*\bedt\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\bedt\.hip\b", mk, re.M)
    assert re.search(r"^ASM :=.*\bedt\b", mk, re.M) and "edt_map.h" in mk
    assert callable(ops.distance_transform) and hasattr(vdr, "morphology") and hasattr(vdr, "metrics")
    assert vdr.segment.MaskDecoder.LAUNCHES == 52
    # 2 bytes a pixel (rounded up to 16 in all) and 8 bytes per 64 x 16 tile of a plane
    assert lib.vdr_distance_transform_workspace_bytes(3, 300, 517) == (2 * 3 * 300 * 517 + 15) // 16 * 16 + 8 * 3 * 9 * 19
    assert lib.vdr_distance_transform_workspace_bytes(1, 1, 1) == 16 + 8
    assert lib.vdr_distance_transform_workspace_bytes(64, 1024, 1024) == (2 + 1 / 128) * 64 * 1024 * 1024
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, 4097), (1, 4097, 4)):
        assert lib.vdr_distance_transform_workspace_bytes(*bad) == 0
    # no atomics in the new file nor in the reduction it shares; components.hip stays the only kernel source with any
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("edt.hip", "edt_map.h", "plane_reduce.h"))
    assert "plane_reduce.h" in mk
    assert not re.search(r"\batomic(Add|Min|Max|CAS|Or)\b|__hip_atomic", text)
    assert "INTEGER ATOMICS live in this file and only here" in open(os.path.join(CSRC, "components.hip")).read()


def test_the_entry_point_refuses_before_the_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 65536)()
    base = (C.addressof(raw) + 255) & ~255
    mk, ws, d2, nr, pk, wi = (base + 4096 * i for i in range(6))

    def dt(mask=mk, P=2, H=8, W=8, value=1, outside=0, r2=0, work=ws, nbytes=4096, d2=d2, nearest=nr, peak=pk, within=wi):
        return lib.vdr_op_distance_transform(mask, P, H, W, value, outside, r2, work, nbytes, d2, nearest, peak, within, None)
    for kw in (dict(mask=None), dict(work=None), dict(d2=None, nearest=None, peak=None, within=None), dict(P=0), dict(P=65536), dict(H=0), dict(H=4097),
               dict(W=0), dict(W=4097), dict(value=2), dict(value=-1), dict(outside=2), dict(outside=-1), dict(outside=1), dict(r2=-1),
               dict(work=ws + 8), dict(d2=d2 + 2), dict(nearest=nr + 1), dict(peak=pk + 3)):
        assert dt(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_distance_transform: "), kw
    need = lib.vdr_distance_transform_workspace_bytes(2, 8, 8)
    assert need == 256 + 16 and dt(nbytes=need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_distance_transform: workspace too small")
    assert dt(outside=1, nearest=None, nbytes=need - 1) == -5 and dt(r2=-1, within=None, nbytes=need - 1) == -5   # r2 is read only with within
    if not torch.cuda.is_available():                                        # VDR_ERR_NO_DEVICE, after every refusal above
        assert dt() == -2 and dt(d2=None, nearest=None, within=None) == -2 and dt(outside=1, nearest=None) == -2


# ---- the Python side ----------------------------------------------------------------------------------------------------------------
def test_ops_and_morphology_refuse_before_any_device_work():
    from vdr import morphology as mo
    from vdr import ops
    m = torch.zeros((2, 8, 8), dtype=torch.uint8)
    for bad in (torch.zeros((8, 8)), torch.zeros((1, 2, 8, 8), dtype=torch.bool), torch.zeros(8, dtype=torch.uint8), np.zeros((8, 8), np.uint8),
                torch.zeros((2, 0, 8), dtype=torch.uint8), torch.zeros((1, 4097), dtype=torch.bool)):
        with pytest.raises(ValueError, match="distance_transform"):
            ops.distance_transform(bad)
        for f in (mo.edt_torch, mo.boundary, mo.signed_distance, mo.inner_point):
            with pytest.raises((ValueError, AttributeError)):
                f(bad)
        with pytest.raises(ValueError, match="dilate"):
            mo.dilate(bad, 2)
    with pytest.raises(ValueError, match="HIP device"):
        ops.distance_transform(m)
    for kw in (dict(value=2), dict(value=True), dict(outside=2), dict(outside="yes"), dict(outside=True, return_nearest=True), dict(threshold=-1),
               dict(threshold=1.5), dict(threshold=True), dict(threshold=2**31), dict(return_d2=False), dict(return_d2=False, return_peak=True, threshold=3)):
        with pytest.raises(ValueError, match="distance_transform: (value|outside|nearest|threshold|return_d2)"):   # on a CPU mask: before the device check
            ops.distance_transform(m, **kw)
    with pytest.raises(ValueError, match="edt_torch"):
        mo.edt_torch(m, outside=True, return_nearest=True)
    for f in (mo.dilate, mo.erode, mo.opening, mo.closing):
        for r in (-1, float("nan"), float("inf"), "2", True, 1e6):
            with pytest.raises(ValueError, match="radius"):
                f(m, r)
    for inner, outer in ((2, 2), (3, 1), (1.0, 1.2), (-1, 2)):
        with pytest.raises(ValueError, match="ring"):
            mo.ring(m, inner, outer)


class _Cfg:
    window, img, patch = 14, 128, 16


def _handle(points=True):
    h = types.SimpleNamespace(model_name="medsam", device="cpu", cfg=_Cfg(), has_mask_decoder=True)
    h.mask_decoder = types.SimpleNamespace(g=8, has_point_prompts=points, has_mask_prompt=True)
    return h


def test_the_layers_above_refuse_before_any_device_work():
    import vdr
    from vdr import pipeline
    x = torch.zeros((3, 3, 128, 128))
    box = torch.tensor([10.0, 10.0, 60.0, 60.0])
    prop = vdr.VitDescriptorModel.propagate_masks
    for bad in ("outer", "Inner", True, 1):
        with pytest.raises(ValueError, match="point_prompt"):
            prop(_handle(), x, box, 1, point_prompt=bad)
        with pytest.raises(ValueError, match="point_prompt"):
            pipeline.propagate_segmentation(None, None, None, None, point_prompt=bad)
    with pytest.raises(ValueError, match="no point-prompt weights .*weights absent"):   # the existing message, before the encoder runs
        prop(_handle(points=False), x, box, 1, point_prompt="inner")
    for f in (pipeline.segment_volume, pipeline.propagate_segmentation):
        for grow in (-1, float("nan"), float("inf"), "3", True):
            with pytest.raises(ValueError, match="grow"):
                f(None, None, None, grow=grow) if f is pipeline.segment_volume else f(None, None, None, None, grow=grow)
    seg = vdr.Segmentation(torch.zeros((1, 2, 1, 32, 32)), torch.zeros((1, 2, 1)), (128, 128))
    vol = vdr.VolumeSegmentation(torch.zeros((3, 32, 32)), torch.zeros(3), torch.zeros((3, 4)), torch.zeros(3, dtype=torch.int32), (128, 128))
    for obj in (seg, vol):
        for kw in (dict(size=(0, 8)), dict(size=(8, 4097)), dict(threshold=float("nan")), dict(threshold="0")):
            with pytest.raises(ValueError, match="distance"):
                obj.distance(**kw)
    # the statements run without a device: an empty volume has no inner point; it matches itself perfectly
    pts, lab = vol.inner_points()
    assert pts.tolist() == [[0.0, 0.0]] * 3 and lab.tolist() == [-1] * 3 and tuple(seg.inner_points()[0].shape) == (1, 2, 1, 2)
    same = vol.compare(vol, size=(40, 40))
    assert same["dice"].tolist() == [1.0] * 3 and same["hd"].tolist() == [0.0] * 3 and same["nsd"].tolist() == [1.0] * 3
    with pytest.raises(ValueError, match="compare"):
        vol.compare(torch.zeros((3, 40, 41), dtype=torch.bool), size=(40, 40))
