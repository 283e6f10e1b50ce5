"""GPU: the exact Euclidean distance transform of mask planes -- vdr_op_distance_transform bit for bit (every output is an integer)
against scipy.ndimage.distance_transform_edt, closed forms and the tie rule restated in numpy (tests/edt_ref.py), on designed
planes that put their features on the seams of the kernels' strips and tiles, on random planes, alone and inside batches, in every
mode, between canaries; then the layers above: vdr.morphology and vdr.metrics on the device against themselves on the CPU, the
inner-point click of propagate_masks against a hand loop, the pipeline's `grow` against scipy.  Nothing is derived from device
output."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import edt_ref as ER
import memguard as mg

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE = ER.NONE
SHAPES = ER.shapes()


@functools.lru_cache(maxsize=None)
def _planes(H, W):
    return ER.planes(H, W)


@functools.lru_cache(maxsize=None)
def _reference(H, W, value, outside):
    """d2 [N, H, W] of every plane of _planes(H, W) by scipy: computed once, shared, never changed"""
    return np.stack([ER.scipy_d2(m, value, outside) for m in _planes(H, W).values()])


@functools.lru_cache(maxsize=None)
def _nearest_reference(H, W, value):
    return np.stack([ER.nearest_given_d2(m, d2, value) for m, d2 in zip(_planes(H, W).values(), _reference(H, W, value, False))])


def _peaks(d2):
    return np.array([ER.peak(p) for p in d2], dtype=np.int32)


def _stack(H, W):
    return torch.from_numpy(np.stack(list(_planes(H, W).values())))


def _eq(got, want, dtype=torch.int32):
    return got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)


# ---- the op -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_distance_transform_equals_scipy_bit_for_bit(H, W):
    """every designed and random plane, the set and the clear pixels, without and with `outside`, every optional output on and
    off, as one batch; then batches of 1, 3 and 5 planes cut from other positions: a plane's outputs depend neither on P nor
    on its position"""
    from vdr import ops
    names = list(_planes(H, W))
    stack = _stack(H, W).to(DEV)
    N = stack.shape[0]
    for value in (0, 1):
        for outside in (False, True):
            want = _reference(H, W, value, outside)
            wp = _peaks(want)
            d2 = ops.distance_transform(stack, value, outside)
            for k, name in enumerate(names):
                assert _eq(d2[k], want[k]), (name, value, outside)
            d2b, peak = ops.distance_transform(stack, value, outside, return_peak=True)
            assert _eq(d2b, want) and _eq(peak, wp), (value, outside)
            for r2 in (0, 1, 2, 10 ** 6):                                    # the thresholded plane instead of d2
                assert _eq(ops.distance_transform(stack, value, outside, threshold=r2), (want <= r2).astype(np.uint8), torch.uint8), (value, outside, r2)
            w2, peak = ops.distance_transform(stack, value, outside, return_peak=True, threshold=2)
            assert _eq(w2, (want <= 2).astype(np.uint8), torch.uint8) and _eq(peak, wp)
            assert _eq(ops.distance_transform(stack, value, outside, return_peak=True, return_d2=False), wp)   # the peak alone
            if not outside:
                wn = _nearest_reference(H, W, value)
                d2c, nearest = ops.distance_transform(stack, value, return_nearest=True)
                assert _eq(d2c, want)
                for k, name in enumerate(names):
                    assert _eq(nearest[k], wn[k]), (name, value)
                d2c, nearest, peak = ops.distance_transform(stack, value, return_nearest=True, return_peak=True)
                assert _eq(d2c, want) and _eq(nearest, wn) and _eq(peak, wp)
                assert _eq(ops.distance_transform(stack, value, return_nearest=True, return_d2=False), wn)     # nearest alone
            for P, s0 in ((1, 0), (1, N - 1), (3, 1), (3, N - 3), (5, 2), (5, N - 5)):
                part = stack[s0:s0 + P].bool() if P == 3 else stack[s0:s0 + P]
                if outside:
                    d, pk = ops.distance_transform(part, value, True, return_peak=True)
                else:
                    d, nr, pk = ops.distance_transform(part, value, return_nearest=True, return_peak=True)
                    assert _eq(nr, _nearest_reference(H, W, value)[s0:s0 + P]), (P, s0, value)
                assert _eq(d, want[s0:s0 + P]) and _eq(pk, wp[s0:s0 + P]), (P, s0, value, outside)
    d = ops.distance_transform(stack[N // 2], 1)                             # a 2-D mask: a 2-D plane back
    assert tuple(d.shape) == (H, W) and _eq(d, _reference(H, W, 1, False)[N // 2])
    d, pk = ops.distance_transform(stack[N // 2].bool(), 1, True, return_peak=True)
    assert tuple(d.shape) == (H, W) and tuple(pk.shape) == (1, 2) and _eq(d, _reference(H, W, 1, True)[N // 2])


@pytest.mark.parametrize("H,W", [(65, 129), (1, 4096), (4096, 1), (300, 517)])
def test_designed_planes_have_their_closed_forms(H, W):
    """what the designs were made for, against closed forms rather than scipy: the full plane, the single clear pixels, the
    checkerboard, the empty plane, the tie rule of nearest"""
    from vdr import ops
    pl = _planes(H, W)
    names = list(pl)
    stack = _stack(H, W).to(DEV)
    d2, nearest, peak = ops.distance_transform(stack, return_nearest=True, return_peak=True)
    d2o, peako = ops.distance_transform(stack, outside=True, return_peak=True)
    yy, xx = np.mgrid[0:H, 0:W]
    k = names.index("full")
    assert bool((d2[k] == NONE).all()) and bool((nearest[k] == -1).all()) and peak[k].tolist() == [NONE, 0]
    assert _eq(d2o[k], ER.closed_form_outside_full(H, W))
    k = names.index("empty")
    assert bool((d2[k] == 0).all()) and bool((nearest[k] == -1).all()) and peak[k].tolist() == [0, -1] and peako[k].tolist() == [0, -1]
    for name, (y0, x0) in (("clear_tl", (0, 0)), ("clear_tr", (0, W - 1)), ("clear_bl", (H - 1, 0)), ("clear_br", (H - 1, W - 1)),
                           ("clear_centre", (H // 2, W // 2))):
        k = names.index(name)
        want = ((yy - y0) ** 2 + (xx - x0) ** 2).astype(np.int32)
        assert _eq(d2[k], want), name
        assert _eq(nearest[k], np.where(want > 0, y0 * W + x0, -1).astype(np.int32)), name
        assert peak[k].tolist() == list(ER.peak(want)), name
    if H > 1 and W > 1:
        k = names.index("checkerboard")
        assert _eq(d2[k], pl["checkerboard"].astype(np.int32))               # every d2 is 1
    if H > 2 and W > 2:
        k = names.index("ties_corners")                                      # equidistant corners: the lowest index wins
        ym, xm = (H - 1) // 2, (W - 1) // 2
        if (H - 1) % 2 == 0:
            assert int(nearest[k, ym, 1]) == 0 and int(nearest[k, ym, W - 2]) == W - 1
        if (W - 1) % 2 == 0:
            assert int(nearest[k, 1, xm]) == 0 and int(nearest[k, H - 2, xm]) == (H - 1) * W


def test_the_peak_reduces_171_tiles_from_the_first_and_the_last():
    """300 x 517 is 171 tiles a plane (19 x 9 of 16 x 64), three trips of the peak kernel's loop over the slots.  Plane 0: 3 x 3 blocks
    in the first and in the last tile and single pixels between them: two equal maxima, the lowest index wins; plane 1: the block
    of the last tile alone is the unique maximum; plane 2: nothing selected, (0, -1).  Exact against vdr.morphology.edt_torch."""
    from vdr import morphology as mo
    from vdr import ops
    H, W = 300, 517
    m = torch.zeros((3, H, W), dtype=torch.uint8)
    m[:2, 296:299, 513:516] = 1                                                # rows 288 .. 299, columns 512 .. 516: the last tile
    m[0, 1:4, 1:4] = 1
    m[:2, 150, ::7] = 1
    want_d2, want_peak = mo.edt_torch(m, return_peak=True)
    assert want_peak.tolist() == [[4, 2 * W + 2], [4, 297 * W + 514], [0, -1]]
    d2, peak = ops.distance_transform(m.to(DEV), return_peak=True)
    assert _eq(d2, want_d2.numpy()) and _eq(peak, want_peak.numpy())
    assert _eq(ops.distance_transform(m.to(DEV), return_peak=True, return_d2=False), want_peak.numpy())   # the peak alone


def test_distance_transform_memory_contract():
    """outputs and workspace of exactly the promised size between canaries; a workspace one byte short is VDR_ERR_WORKSPACE with
    the canary-filled outputs untouched; null optional outputs are not touched (whatever is not asked for stays canary)"""
    from vdr import _lib
    lib = _lib.load()
    P, H, W = 3, 67, 131
    m = torch.from_numpy(np.stack([ER.bernoulli(H, W, p, 3) for p in (0.5, 0.99, 0.999)]))
    dev = m.to(DEV)
    need = lib.vdr_distance_transform_workspace_bytes(P, H, W)
    assert need == (2 * P * H * W + 15) // 16 * 16 + 8 * P * 3 * 5
    stream = torch.cuda.current_stream().cuda_stream
    want = np.stack([ER.scipy_d2(m[p].numpy()) for p in range(P)])
    wn = np.stack([ER.nearest_given_d2(m[p].numpy(), want[p]) for p in range(P)])
    for asked in ("d2 nearest peak within", "d2", "within", "peak", "nearest", "d2 peak"):
        wd, d2 = mg.guarded(4 * P * H * W, 256)
        wnr, nearest = mg.guarded(4 * P * H * W, 256)
        wp, peak = mg.guarded(8 * P, 256)
        ww, within = mg.guarded(P * H * W, 256)
        wk, work = mg.guarded(need, 256)
        ptr = {n: (t.data_ptr() if n in asked.split() else None) for n, t in (("d2", d2), ("nearest", nearest), ("peak", peak), ("within", within))}

        def call(nbytes):
            return lib.vdr_op_distance_transform(dev.data_ptr(), P, H, W, 1, 0, 5, work.data_ptr(), nbytes, ptr["d2"], ptr["nearest"], ptr["peak"],
                                                 ptr["within"], stream)
        assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_distance_transform: workspace too small")
        torch.cuda.synchronize()
        assert mg.canary_left(d2.view(torch.int32)) == P * H * W and mg.canary_left(nearest.view(torch.int32)) == P * H * W
        assert mg.canary_left(peak.view(torch.int32)) == 2 * P and mg.canary_left(within) == P * H * W and mg.canary_left(work) == need
        assert call(need) == 0
        torch.cuda.synchronize()
        assert all(mg.guards_intact(w, 256) for w in (wd, wnr, wp, ww, wk)), asked
        got = {"d2": (d2.view(torch.int32), want.reshape(-1)), "nearest": (nearest.view(torch.int32), wn.reshape(-1)),
               "peak": (peak.view(torch.int32), _peaks(want).reshape(-1)), "within": (within, (want <= 5).astype(np.uint8).reshape(-1))}
        for n, (t, w) in got.items():
            if n in asked.split():
                assert np.array_equal(t.cpu().numpy(), w), (asked, n)
            else:
                assert mg.canary_left(t) == t.numel(), (asked, n)             # not asked for: not touched


# ---- vdr.morphology and vdr.metrics on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (17, 63), (65, 129)])
def test_morphology_on_the_device_equals_itself_on_the_cpu(H, W):
    """every function on the designed planes, device against CPU statement, bit for bit (the CPU statement is held to scipy in
    tests/test_edt_cpu.py); inner_point lies inside its mask and on the peak"""
    from vdr import morphology as mo
    cpu = _stack(H, W)
    dev = cpu.to(DEV)
    for r in (1, 1.5, 3.5, 9):
        for name, f in (("dilate", mo.dilate), ("erode", mo.erode), ("opening", mo.opening), ("closing", mo.closing),
                        ("erode_inside", lambda m, r: mo.erode(m, r, outside=False)), ("closing_scipy", lambda m, r: mo.closing(m, r, outside=True))):
            got, want = f(dev, r), f(cpu, r)
            assert got.dtype == want.dtype == torch.uint8 and torch.equal(got.cpu(), want), (name, r)
        assert mo.dilate(dev.bool(), r).dtype == torch.bool
    assert mo.dilate(dev, 0) is dev
    assert torch.equal(mo.ring(dev, 1.5, 4).cpu(), mo.ring(cpu, 1.5, 4)) and torch.equal(mo.boundary(dev).cpu(), mo.boundary(cpu))
    sd, sc = mo.signed_distance(dev), mo.signed_distance(cpu)
    assert sd.dtype == torch.float32 and torch.equal(sd.cpu(), sc)
    for outside in (True, False):
        for img in (None, 4 * max(H, W), (3 * H, 5 * W)):
            (pd, ld), (pc, lc) = mo.inner_point(dev, img, outside), mo.inner_point(cpu, img, outside)
            assert pd.dtype == torch.float32 and ld.dtype == torch.int32 and torch.equal(pd.cpu(), pc) and torch.equal(ld.cpu(), lc)
    pts, lab = mo.inner_point(dev)
    want = _reference(H, W, 1, True)
    for k, (name, m) in enumerate(_planes(H, W).items()):
        x, y = (int(v) for v in pts[k].tolist())
        if m.any():
            assert int(lab[k]) == 1 and m[y, x] and want[k, y, x] == want[k].max(), name
        else:
            assert int(lab[k]) == -1 and (x, y) == (0, 0), name


def test_metrics_on_the_device_equal_the_cpu_values():
    """integer counts and hd equal (the same integers, the same IEEE sqrt); the float64 means and percentiles within rtol 1e-12
    (a few float64 roundings; the order of a sum may differ between the devices)"""
    from vdr import metrics
    pl = _planes(65, 129)
    a = torch.from_numpy(np.stack([pl["bernoulli0.5"], 1 - pl["clear_row"], pl["seams"], pl["empty"], pl["empty"], pl["full"]])).bool()
    yy, xx = np.mgrid[0:65, 0:129]
    blob = lambda cy, cx, r: (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r    # noqa: E731
    a = torch.cat([a, torch.from_numpy(np.stack([blob(30, 60, 20), blob(20, 40, 12) | blob(40, 90, 15)]))])
    b = torch.cat([a[1:], a[:1]])
    b[-1] = torch.from_numpy(blob(33, 57, 22))
    b[3] = False                                                              # empty against empty
    for spacing, tol in ((1.0, 1.0), (0.7, 2.0)):
        oc, od = metrics.overlap(a, b), metrics.overlap(a.to(DEV), b.to(DEV))
        sc, sd = metrics.surface(a, b, spacing, tol), metrics.surface(a.to(DEV), b.to(DEV), spacing, tol)
        for n in ("intersection", "a", "b", "dice", "iou"):
            assert torch.equal(od[n].cpu(), oc[n]), n
        assert torch.equal(sd["hd"].cpu(), sc["hd"])
        for n in ("hd95", "assd", "nsd"):
            g, w = sd[n].cpu(), sc[n]
            assert g.dtype == torch.float64 and bool(((g == w) | ((g - w).abs() <= 1e-12 * w.abs())).all()), (n, g, w)
    assert float(sc["nsd"][3]) == 1.0 and float(sc["hd"][4]) == float("inf")   # two empty masks; one empty mask


# ---- the layers above: the tiny seeded SAM of tests/handle_configs.py with the prompt golden's decoder -----------------------------------
@contextlib.contextmanager
def _sam(base, name, drop=()):
    import handle_configs as hc
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(base["cfg"].img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS[name] = hc.sam_config(cfg)
    try:
        w = dict(so.make_weights(cfg, seed=base["wseed"], scale=0.05))
        w.update({k: v for k, v in base["weights"].items() if not k.startswith(drop)})
        yield vdr.load_model(name, weights=w, decoder_eps=base["eps"])
    finally:
        del vdr.ARCHS[name]


@pytest.fixture(scope="module")
def base(golden_dir):
    import sam_prompt_ref as PR
    return PR.golden_prompts(golden_dir, "g8")[0]


@pytest.fixture(scope="module")
def model(base):
    with _sam(base, "sam_edt_g8") as m:
        yield m


@pytest.fixture(scope="module")
def volume(base):
    x = torch.cat([base["image"], base["image"].flip(-1), base["image"][:1].flip(-2)], dim=0).to(DEV)   # Z = 5 slices [5, 3, 128, 128]
    return x, torch.tensor([20.0, 30.0, 90.0, 100.0])


def _hand_loop(m, x, box, index, order, margin, max_batch):
    """decode_masks slice by slice with the box, the mask prompt and the click -- the click from the CPU statement of inner_point
    on the neighbour's token-0 mask -- and the torch statement of mask_box"""
    import sam_prompt_ref as PR
    from vdr import morphology as mo
    emb = torch.cat([m.image_encoder(x[s0:s0 + max_batch]) for s0 in range(0, x.shape[0], max_batch)], dim=0)
    out, clicks = {}, {}
    state = None
    for z in [index] + list(order):
        if z == index:
            used = box.to(DEV).float()
            seg = m.decode_masks(emb[z:z + 1], box.reshape(1, 1, 4))
        else:
            used = state[1]
            pts, lab = mo.inner_point((state[0] > 0).cpu(), m.cfg.img, outside=True)          # the CPU statement
            clicks[z] = (pts[0].tolist(), int(lab[0]))
            seg = m.decode_masks(emb[z:z + 1], used.reshape(1, 1, 4), points=pts.reshape(1, 1, 1, 2), point_labels=lab.reshape(1, 1, 1),
                                 mask_input=state[0].reshape(1, 1, *state[0].shape))
        lg = seg.low_res_logits[0, 0, 0]
        nxt, area = PR.mask_box_ref(lg[None], used[None], m.cfg.img, margin, 0.0)
        out[z] = (lg, seg.iou[0, 0, 0], used, area[0])
        state = (lg, nxt[0])
    return out, clicks


def test_propagate_masks_with_the_inner_click_equals_a_hand_loop_bit_for_bit(base, model, volume):
    m, (x, box) = model, volume
    assert m.mask_decoder.LAUNCHES == 52
    plain = m.propagate_masks(x, box, 2, max_batch=2)
    none = m.propagate_masks(x, box, 2, max_batch=2, point_prompt=None)
    for f in ("low_res_logits", "iou", "boxes", "area"):
        assert torch.equal(getattr(plain, f), getattr(none, f)), f                             # None is the call without the keyword
    vol = m.propagate_masks(x, box, 2, max_batch=2, point_prompt="inner")
    up, clicks = _hand_loop(m, x, box, 2, [3, 4], 8.0, 2)
    down, clicks_down = _hand_loop(m, x, box, 2, [1, 0], 8.0, 2)
    want = dict(up)
    want.update({z: v for z, v in down.items() if z < 2})
    for z in range(5):
        lg, iou, used, area = want[z]
        assert torch.equal(vol.low_res_logits[z], lg) and torch.equal(vol.iou[z], iou), z
        assert torch.equal(vol.boxes[z], used) and int(vol.area[z]) == int(area), z
    print("clicks", clicks, clicks_down)
    assert any(lab == 1 for _, lab in list(clicks.values()) + list(clicks_down.values()))       # the sweep did click
    assert not torch.equal(vol.low_res_logits[3], plain.low_res_logits[3])                     # and the click reached the decoder
    # the objects' own accessors against the CPU statements
    from vdr import morphology as mo
    pts, lab = vol.inner_points()
    pc, lc = mo.inner_point((vol.low_res_logits > 0).cpu(), m.cfg.img, outside=True)
    assert torch.equal(pts.cpu(), pc) and torch.equal(lab.cpu(), lc)
    from vdr import amg
    d2 = vol.distance(size=(50, 70))
    raw = amg.upsample_torch(vol.low_res_logits.cpu(), (50, 70)) > 0.0
    assert d2.dtype == torch.int32 and np.array_equal(d2.cpu().numpy(), np.stack([ER.scipy_d2(p.numpy()) for p in raw]))
    seg = m.segment(x[:2], box.reshape(1, 1, 4).expand(2, 1, 4), multimask=True)
    sp, sl = seg.inner_points()
    pc, lc = mo.inner_point((seg.low_res_logits > 0).flatten(0, 2).cpu(), m.cfg.img, outside=True)
    assert tuple(sp.shape) == (2, 1, 3, 2) and torch.equal(sp.cpu().reshape(-1, 2), pc) and torch.equal(sl.cpu().reshape(-1), lc)
    assert tuple(seg.distance().shape) == (2, 1, 3, 128, 128)
    # compare: the device route against the CPU one
    from vdr import metrics
    got = vol.compare(plain, size=(50, 70))
    a, b = vol.masks((50, 70)).cpu(), plain.masks((50, 70)).cpu()
    wo, ws = metrics.overlap(a, b), metrics.surface(a, b)
    for n in ("intersection", "a", "b", "dice", "iou"):
        assert torch.equal(got[n].cpu(), wo[n]), n
    assert torch.equal(got["hd"].cpu(), ws["hd"])
    for n in ("hd95", "assd", "nsd"):
        g, w = got[n].cpu(), ws[n]
        assert bool(((g == w) | ((g - w).abs() <= 1e-12 * w.abs())).all()), n
    with _sam(base, "sam_edt_box_only", drop=("prompt_encoder.not_a_point_embed",)) as box_only:
        with pytest.raises(ValueError, match="weights absent"):
            box_only.propagate_masks(x, box, 2, point_prompt="inner")
        assert torch.equal(box_only.propagate_masks(x, box, 2, max_batch=2).low_res_logits, plain.low_res_logits)   # without the click it runs


def test_pipeline_grow_is_scipys_dilation_of_the_old_array(model):
    import vdr
    from scipy import ndimage
    m = model
    H, W, S = 96, 80, 5
    vol = torch.rand((H, W, S), generator=torch.Generator().manual_seed(71)).numpy().astype(np.float32)
    box = np.array([20.0, 25.0, 60.0, 70.0])
    calls = ((vdr.pipeline.segment_volume, (m, vol, box), dict(max_batch=2)),
             (vdr.pipeline.propagate_segmentation, (m, vol, box, 2), dict(max_batch=2)),
             (vdr.pipeline.propagate_segmentation, (m, vol, box, 2), dict(max_batch=2, min_region_area=20)))
    for f, args, kw in calls:
        old = f(*args, **kw)
        assert old.any() and np.array_equal(f(*args, grow=0, **kw), old) and np.array_equal(f(*args, grow=0.0, **kw), old)
        for grow in (3, 2.5):
            got = f(*args, grow=grow, **kw)
            want = np.stack([ndimage.binary_dilation(old[:, :, s], ER.disc(grow)) for s in range(S)], axis=2)
            assert got.dtype == np.bool_ and got.shape == (H, W, S) and np.array_equal(got, want), (f.__name__, grow)
    a = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2, point_prompt="inner")
    b = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2)
    assert a.shape == b.shape and np.array_equal(a[:, :, 2], b[:, :, 2])                       # the annotated slice has no click
