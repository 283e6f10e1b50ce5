"""GPU: the exact 3-D Euclidean distance transform with voxel spacing -- vdr_op_distance_transform_3d bit for bit (every output is
an integer) against scipy.ndimage.distance_transform_edt(sampling=) (tests/edt3d_ref.py), on designed and random volumes, alone
and inside batches, in every mode, between canaries; then the layers above: vdr.morphology and vdr.metrics with a spacing on the
device against themselves on the CPU (held to scipy in tests/test_edt3d_cpu.py), VolumeSegmentation.compare / distance, the
pipeline's `grow` with `spatial_res` against scipy's ellipsoid, and spacing=None / spatial_res=None against the slice-by-slice
path.  Nothing is derived from device output."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import edt3d_ref as E3
import memguard as mg

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE = E3.NONE
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 5, 9), (3, 17, 65), (9, 16, 64), (33, 24, 19), (70, 5, 130)]
OUTSIDES = (0, 7, 4, 3)


@functools.lru_cache(maxsize=None)
def _volumes(shape):
    return E3.volumes(*shape)


@functools.lru_cache(maxsize=None)
def _reference(shape, q, value, outside):
    """d2 [N, Z, H, W] of every volume of _volumes(shape) by scipy: computed once, shared, never changed"""
    return np.stack([E3.scipy_d2(m, q, value, outside) for m in _volumes(shape).values()])


def _peaks(d2):
    return np.array([E3.peak(p) for p in d2], dtype=np.int64)


def _eq(got, want, dtype=torch.int64):
    return got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)


# ---- the op -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_distance_transform_3d_equals_scipy_bit_for_bit(shape):
    """every designed and random volume, every spacing, the set and the clear voxels, `outside` 0, 7, 4 and 3, every optional output
    on and off, r2 in {0, 1, qx^2, 10^12}, as one batch; then batches of 1, 3 and 5 volumes cut from other positions: a volume's
    outputs depend neither on P nor on its position"""
    from vdr import ops
    names = list(_volumes(shape))
    stack = torch.from_numpy(np.stack(list(_volumes(shape).values()))).to(DEV)
    N = stack.shape[0]
    for q in E3.SPACINGS:
        assert E3.exact(shape, q)
        for value in (0, 1):
            for outside in OUTSIDES:
                o3 = E3.bits3(outside)
                want = _reference(shape, q, value, outside)
                wp = _peaks(want)
                d2 = ops.distance_transform_3d(stack, q, value, o3)
                for k, name in enumerate(names):
                    assert _eq(d2[k], want[k]), (name, q, value, outside)
                d2b, peak = ops.distance_transform_3d(stack, q, value, o3, return_peak=True)
                assert _eq(d2b, want) and _eq(peak, wp), (q, value, outside)
                for r2 in (0, 1, q[2] ** 2, 10 ** 12):                          # the thresholded volume instead of d2: the early exits
                    got = ops.distance_transform_3d(stack, q, value, o3, threshold=r2)
                    assert _eq(got, (want <= r2).astype(np.uint8), torch.uint8), (q, value, outside, r2)
                w2, peak = ops.distance_transform_3d(stack, q, value, o3, return_peak=True, threshold=q[2] ** 2)   # with the peak: the full search
                assert _eq(w2, (want <= q[2] ** 2).astype(np.uint8), torch.uint8) and _eq(peak, wp)
                assert _eq(ops.distance_transform_3d(stack, q, value, o3, return_peak=True, return_d2=False), wp)   # the peak alone
                for P, s0 in ((1, 0), (1, N - 1), (3, 1), (3, N - 3), (5, 2), (5, N - 5)):
                    part = stack[s0:s0 + P].bool() if P == 3 else stack[s0:s0 + P]
                    d, pk = ops.distance_transform_3d(part, q, value, o3, return_peak=True)
                    assert _eq(d, want[s0:s0 + P]) and _eq(pk, wp[s0:s0 + P]), (P, s0, q, value, outside)
                    assert _eq(ops.distance_transform_3d(part, q, value, o3, threshold=q[1] ** 2), (want[s0:s0 + P] <= q[1] ** 2).astype(np.uint8), torch.uint8)
    d = ops.distance_transform_3d(stack[N // 2], (3, 1, 1))                   # a 3-D mask: a 3-D volume back
    assert tuple(d.shape) == shape and _eq(d, _reference(shape, (3, 1, 1), 1, 0)[N // 2])
    d, pk = ops.distance_transform_3d(stack[N // 2].bool(), (3, 1, 1), 1, True, return_peak=True)
    assert tuple(d.shape) == shape and tuple(pk.shape) == (1, 2) and _eq(d, _reference(shape, (3, 1, 1), 1, 7)[N // 2])
    k = names.index("all_set")                                               # no candidate at all
    d2, peak = ops.distance_transform_3d(stack[k], (1, 2, 5), return_peak=True)
    assert bool((d2 == NONE).all()) and peak.tolist() == [[NONE, 0]]
    assert ops.distance_transform_3d(stack[names.index("none_set")], return_peak=True)[1].tolist() == [[0, -1]]


def test_the_search_depth_at_its_limit():
    """4096 x 1 x 2 with one clear voxel, 8 K voxels: the z search walks up to 4095 slices.  (65535, 1, 300) is beyond the
    exactness bound at this depth and is refused before the device."""
    from vdr import ops
    shape = (4096, 1, 2)
    for corner in ((0, 0, 0), (4095, 0, 1), (2048, 0, 0)):
        m = np.ones(shape, np.uint8)
        m[corner] = 0
        t = torch.from_numpy(m).to(DEV)
        for q in E3.SPACINGS:
            if not E3.exact(shape, q):
                assert q == (65535, 1, 300)
                with pytest.raises(ValueError, match="2\\^53"):
                    ops.distance_transform_3d(t, q)
                continue
            for outside in OUTSIDES:
                want = E3.scipy_d2(m, q, 1, outside)
                d2, peak = ops.distance_transform_3d(t, q, 1, E3.bits3(outside), return_peak=True)
                assert _eq(d2, want) and peak.tolist() == [list(E3.peak(want))], (corner, q, outside)
                for r2 in (0, 1, q[2] ** 2, 10 ** 12):
                    assert _eq(ops.distance_transform_3d(t, q, 1, E3.bits3(outside), threshold=r2), (want <= r2).astype(np.uint8), torch.uint8)
            assert _eq(ops.distance_transform_3d(t, q, 0), np.where(m == 0, min(q[0], q[2]) ** 2, 0).astype(np.int64))   # the lone clear voxel: a z or an x neighbour


def test_the_peak_reduces_many_tiles_from_the_first_and_the_last():
    """40 x 20 x 130 is 40 slices of 2 x 3 tiles: 240 slots a volume, four trips of the finish kernel's loop.  Volume 0: equal cubes in
    the first and in the last tile and single voxels between them: two equal maxima, the lowest index wins; volume 1: the cube of the
    last tile alone; volume 2: nothing selected, (0, -1).  Exact against vdr.morphology.edt3d_torch."""
    from vdr import morphology as mo
    from vdr import ops
    Z, H, W = 40, 20, 130
    m = torch.zeros((3, Z, H, W), dtype=torch.uint8)
    m[:2, 36:39, 16:19, 126:129] = 1
    m[0, 1:4, 1:4, 1:4] = 1
    m[:2, 20, 10, ::7] = 1
    want_d2, want_peak = mo.edt3d_torch(m, (2, 2, 2), return_peak=True)
    assert want_peak.tolist() == [[16, (2 * H + 2) * W + 2], [16, (37 * H + 17) * W + 127], [0, -1]]
    d2, peak = ops.distance_transform_3d(m.to(DEV), (2, 2, 2), return_peak=True)
    assert _eq(d2, want_d2.numpy()) and _eq(peak, want_peak.numpy())
    assert _eq(ops.distance_transform_3d(m.to(DEV), (2, 2, 2), return_peak=True, return_d2=False), want_peak.numpy())


def test_distance_transform_3d_memory_contract():
    """outputs and workspace of exactly the promised size between canaries; a workspace one byte short is VDR_ERR_WORKSPACE with
    the canary-filled outputs untouched; null optional outputs are not touched (whatever is not asked for stays canary)"""
    from vdr import _lib
    lib = _lib.load()
    P, Z, H, W = 3, 5, 19, 67
    n = P * Z * H * W
    m = np.stack([E3.bernoulli((Z, H, W), p, 3) for p in (0.5, 0.99, 0.999)])
    dev = torch.from_numpy(m).to(DEV)
    q, outside, r2 = (2560, 717, 717), 4, 3 * 2560 ** 2
    need = lib.vdr_distance_transform_3d_workspace_bytes(P, Z, H, W)
    assert need == (2 * n + 15) // 16 * 16 + (4 * n + 15) // 16 * 16 + 16 * P * Z * 2 * 2
    stream = torch.cuda.current_stream().cuda_stream
    want = np.stack([E3.scipy_d2(m[p], q, 1, outside) for p in range(P)])
    for asked in ("d2 peak within", "d2", "within", "peak", "d2 peak", "within peak"):
        wd, d2 = mg.guarded(8 * n, 256)
        wp, peak = mg.guarded(16 * P, 256)
        ww, within = mg.guarded(n, 256)
        wk, work = mg.guarded(need, 256)
        ptr = {k: (t.data_ptr() if k in asked.split() else None) for k, t in (("d2", d2), ("peak", peak), ("within", within))}

        def call(nbytes):
            return lib.vdr_op_distance_transform_3d(dev.data_ptr(), P, Z, H, W, q[0], q[1], q[2], 1, outside, r2, work.data_ptr(), nbytes, ptr["d2"],
                                                    ptr["peak"], ptr["within"], stream)
        assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_distance_transform_3d: workspace too small")
        torch.cuda.synchronize()
        assert mg.canary_left(d2.view(torch.int64)) == n and mg.canary_left(peak.view(torch.int64)) == 2 * P
        assert mg.canary_left(within) == n and mg.canary_left(work) == need
        assert call(need) == 0
        torch.cuda.synchronize()
        assert all(mg.guards_intact(w, 256) for w in (wd, wp, ww, wk)), asked
        got = {"d2": (d2.view(torch.int64), want.reshape(-1)), "peak": (peak.view(torch.int64), _peaks(want).reshape(-1)),
               "within": (within, (want <= r2).astype(np.uint8).reshape(-1))}
        for k, (t, w) in got.items():
            if k in asked.split():
                assert np.array_equal(t.cpu().numpy(), w), (asked, k)
            else:
                assert mg.canary_left(t) == t.numel(), (asked, k)             # not asked for: not touched


# ---- vdr.morphology and vdr.metrics on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 17, 63), (9, 20, 70)])
def test_morphology_with_spacing_on_the_device_equals_itself_on_the_cpu(shape):
    """every function on the designed volumes, device against CPU statement, bit for bit (the CPU statement is held to scipy in
    tests/test_edt3d_cpu.py); inner_voxel lies inside its mask and on the peak; spacing=None is the 2-D path"""
    from vdr import morphology as mo
    cpu = torch.from_numpy(np.stack(list(_volumes(shape).values())))
    dev = cpu.to(DEV)
    for spacing in ((2.5, 0.7, 0.7), (1.0, 1.0, 1.0)):
        for r in (0.5, 1.0, 3.0, 9.0):
            for name, f in (("dilate", mo.dilate), ("erode", mo.erode), ("opening", mo.opening), ("closing", mo.closing),
                            ("erode_inside", lambda m, r, spacing: mo.erode(m, r, outside=False, spacing=spacing)),
                            ("erode_z", lambda m, r, spacing: mo.erode(m, r, outside=(True, False, False), spacing=spacing))):
                got, want = f(dev, r, spacing=spacing), f(cpu, r, spacing=spacing)
                assert got.dtype == want.dtype == torch.uint8 and torch.equal(got.cpu(), want), (name, r, spacing)
            assert mo.dilate(dev.bool(), r, spacing=spacing).dtype == torch.bool
        assert mo.dilate(dev, 0, spacing=spacing) is dev
        assert torch.equal(mo.ring(dev, 1.5, 4, spacing=spacing).cpu(), mo.ring(cpu, 1.5, 4, spacing=spacing))
        assert torch.equal(mo.boundary(dev, spacing=spacing).cpu(), mo.boundary(cpu, spacing=spacing))
        sd, sc = mo.signed_distance(dev, spacing=spacing), mo.signed_distance(cpu, spacing=spacing)
        assert sd.dtype == torch.float32 and torch.equal(sd.cpu(), sc)
        for outside in (True, False, (True, False, False)):
            (zd, ld), (zc, lc) = mo.inner_voxel(dev, spacing, outside), mo.inner_voxel(cpu, spacing, outside)
            assert zd.dtype == torch.int64 and ld.dtype == torch.int32 and torch.equal(zd.cpu(), zc) and torch.equal(ld.cpu(), lc)
    zyx, lab = mo.inner_voxel(dev, (2.5, 0.7, 0.7))
    want = _reference(shape, (2560, 717, 717), 1, 7)
    for k, (name, m) in enumerate(_volumes(shape).items()):
        z, y, x = (int(v) for v in zyx[k].tolist())
        if m.any():
            assert int(lab[k]) == 1 and m[z, y, x] and want[k, z, y, x] == want[k].max(), name
        else:
            assert int(lab[k]) == -1 and (z, y, x) == (0, 0, 0), name
    planes = dev.reshape(-1, shape[1], shape[2])                              # spacing=None: today's path and today's bits
    for f in (mo.dilate, mo.erode, mo.opening, mo.closing):
        assert torch.equal(f(planes, 1.5, spacing=None), f(planes, 1.5))
    assert torch.equal(mo.boundary(planes, spacing=None), mo.boundary(planes)) and torch.equal(mo.ring(planes, 1, 3, spacing=None), mo.ring(planes, 1, 3))
    with pytest.raises(ValueError, match="dilate"):
        mo.dilate(dev, 1.5)                                                  # a 4-D input without spacing stays refused


def test_surface_measures_of_volumes_on_the_device_equal_the_cpu_values():
    """integer counts, hd and nsd equal (the same integers, the same IEEE sqrt, an integer comparison); the float64 means and
    percentiles within rtol 1e-12 (a few float64 roundings; the order of a sum may differ between the devices)"""
    from vdr import metrics
    Z, H, W = 9, 33, 41
    zz, yy, xx = np.mgrid[0:Z, 0:H, 0:W]
    blob = lambda cz, cy, cx, r: (2.5 * (zz - cz)) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r    # noqa: E731
    a = torch.from_numpy(np.stack([blob(4, 16, 20, 9), blob(3, 10, 12, 6) | blob(5, 22, 30, 7), E3.bernoulli((Z, H, W), 0.5, 1) != 0,
                                   np.zeros((Z, H, W), bool), np.zeros((Z, H, W), bool), np.ones((Z, H, W), bool)]))
    b = torch.cat([a[1:], a[:1]])
    b[0] = torch.from_numpy(blob(4, 18, 18, 10))
    b[3] = False                                                              # empty against empty
    for spacing, tol in (((2.5, 0.7, 0.7), 1.0), ((1.0, 1.0, 1.0), 2.0)):
        oc, od = metrics.overlap(a, b, volumes=True), metrics.overlap(a.to(DEV), b.to(DEV), volumes=True)
        sc, sd = metrics.surface(a, b, spacing, tol), metrics.surface(a.to(DEV), b.to(DEV), spacing, tol)
        for n in ("intersection", "a", "b", "dice", "iou"):
            assert torch.equal(od[n].cpu(), oc[n]), n
        assert torch.equal(sd["hd"].cpu(), sc["hd"]) and torch.equal(sd["nsd"].cpu(), sc["nsd"])
        for n in ("hd95", "assd"):
            g, w = sd[n].cpu(), sc[n]
            assert g.dtype == torch.float64 and bool(((g == w) | ((g - w).abs() <= 1e-12 * w.abs())).all()), (n, g, w)
        want = E3.surface_scipy(a[0].numpy(), b[0].numpy(), spacing, tol)     # and one of them against scipy directly
        assert float(sd["hd"][0]) == want["hd"] and float(sd["nsd"][0]) == want["nsd"]
    assert float(sc["nsd"][3]) == 1.0 and float(sc["hd"][4]) == float("inf")   # two empty masks; one empty mask


# ---- the layers above: the tiny seeded SAM of tests/handle_configs.py with the prompt golden's decoder -----------------------------------
@contextlib.contextmanager
def _sam(base, name):
    import handle_configs as hc
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(base["cfg"].img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS[name] = hc.sam_config(cfg)
    try:
        w = dict(so.make_weights(cfg, seed=base["wseed"], scale=0.05))
        w.update(base["weights"])
        yield vdr.load_model(name, weights=w, decoder_eps=base["eps"])
    finally:
        del vdr.ARCHS[name]


@pytest.fixture(scope="module")
def base(golden_dir):
    import sam_prompt_ref as PR
    return PR.golden_prompts(golden_dir, "g8")[0]


@pytest.fixture(scope="module")
def model(base):
    with _sam(base, "sam_edt3d_g8") as m:
        yield m


def test_volume_segmentation_compare_and_distance_with_spacing(base, model):
    from vdr import amg, metrics
    m = model
    x = torch.cat([base["image"], base["image"].flip(-1), base["image"][:1].flip(-2)], dim=0).to(DEV)   # Z = 5 slices
    box = torch.tensor([20.0, 30.0, 90.0, 100.0])
    plain = m.propagate_masks(x, box, 2, max_batch=2)
    other = m.propagate_masks(x, box, 1, max_batch=2)
    spacing = (2.5, 0.7, 0.7)
    got = plain.compare(other, size=(50, 70), spacing=spacing, tolerance=1.5)
    a, b = plain.masks((50, 70)).cpu(), other.masks((50, 70)).cpu()
    wo, ws = metrics.overlap(a, b, volumes=True), metrics.surface(a, b, spacing=spacing, tolerance=1.5)
    for n in ("intersection", "a", "b", "dice", "iou"):
        assert tuple(got[n].shape) == (1,) and torch.equal(got[n].cpu(), wo[n]), n
    assert torch.equal(got["hd"].cpu(), ws["hd"]) and torch.equal(got["nsd"].cpu(), ws["nsd"])
    for n in ("hd95", "assd"):
        g, w = got[n].cpu(), ws[n]
        assert bool(((g == w) | ((g - w).abs() <= 1e-12 * w.abs())).all()), n
    want = E3.surface_scipy(a.numpy(), b.numpy(), spacing, 1.5)
    assert float(got["hd"][0]) == want["hd"]
    old = plain.compare(other, size=(50, 70))                                 # without a 3-sequence: slice by slice, as before
    assert tuple(old["hd"].shape) == (5,) and torch.equal(old["hd"].cpu(), metrics.surface(a, b)["hd"])
    d2 = plain.distance(size=(50, 70), spacing=spacing)
    raw = (amg.upsample_torch(plain.low_res_logits.cpu(), (50, 70)) > 0.0).numpy()
    assert d2.dtype == torch.int64 and np.array_equal(d2.cpu().numpy(), E3.scipy_d2(raw, (2560, 717, 717)))
    assert plain.distance(size=(50, 70)).dtype == torch.int32                 # and the 2-D one is what it was


def test_pipeline_grow_with_spatial_res_is_scipys_ellipsoid_over_the_volume(model):
    import vdr
    from scipy import ndimage
    m = model
    H, W, S = 96, 80, 5
    vol = torch.rand((H, W, S), generator=torch.Generator().manual_seed(71)).numpy().astype(np.float32)
    box = np.array([20.0, 25.0, 60.0, 70.0])
    res = (0.7, 0.8, 2.5)                                                     # (x, y, z), the reference's order
    q = E3.quantize((2.5, 0.8, 0.7))
    calls = ((vdr.pipeline.segment_volume, (m, vol, box), dict(max_batch=2)),
             (vdr.pipeline.propagate_segmentation, (m, vol, box, 2), dict(max_batch=2)))
    for f, args, kw in calls:
        old = f(*args, **kw)
        assert old.any() and np.array_equal(f(*args, spatial_res=None, **kw), old)
        assert np.array_equal(f(*args, grow=0, spatial_res=res, **kw), old) and np.array_equal(f(*args, grow=0.5, spatial_res=res, **kw), old)
        slicewise = f(*args, grow=2.5, **kw)                                 # spatial_res=None: the parent's path, bit for bit
        assert np.array_equal(f(*args, grow=2.5, spatial_res=None, **kw), slicewise)
        r2d = int(np.floor(2.5 * 2.5))
        k = int(np.floor(np.sqrt(r2d)))
        yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
        assert np.array_equal(slicewise, np.stack([ndimage.binary_dilation(old[:, :, s], yy * yy + xx * xx <= r2d) for s in range(S)], axis=2))
        for grow in (3, 2.5, 0.75):
            got = f(*args, grow=grow, spatial_res=res, **kw)
            zhw = np.ascontiguousarray(old.transpose(2, 0, 1))
            want = ndimage.binary_dilation(zhw, E3.ellipsoid(q, E3.radius2(grow), zhw.shape)).transpose(1, 2, 0)
            assert got.dtype == np.bool_ and got.shape == (H, W, S) and np.array_equal(got, want), (f.__name__, grow)
