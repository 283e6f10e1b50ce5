"""GPU: connected components of mask planes -- vdr_op_connected_components, vdr_op_mask_clean and vdr_op_mask_binarize bit for bit
(every output is an integer) against scipy.ndimage.label and the clean rules restated on top of it (tests/components_ref.py),
on designed planes that put their features on the seams of the kernels' 64 x 64 tiles, on random planes near the percolation
thresholds, alone and inside batches, between canaries; then the layers above: Segmentation.clean, the pipeline keywords,
generate_masks(min_mask_region_area) and the device labelling of TokenCut / LOST.  Nothing is derived from device output."""
import functools

import numpy as np
import pytest
import torch

import components_ref as CR
import memguard as mg

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = CR.T
SIDES = (1, 2, T - 1, T, T + 1, 2 * T + 1)
# every side against every side once (a Latin arrangement: each value occurs as H and as W with several partners, the non-square
# pairs included), then the two planes of the issue
SHAPES = [(1, 1), (1, 2 * T + 1), (2, T), (2, 2), (T - 1, T + 1), (T - 1, 1), (T, T), (T, 2), (T + 1, T - 1), (T + 1, T + 1), (2 * T + 1, T),
          (2 * T + 1, 2 * T + 1), (T + 1, 2 * T + 1), (129, 257), (300, 517)]


def _roots(mask, conn, value):
    """the reference: scipy.ndimage.label's partition (the numpy union-find states the same one where scipy is absent; the CPU
    tests hold the two equal)"""
    try:
        return CR.scipy_roots(mask, conn, value)
    except ImportError:
        return CR.roots_union_find(mask, conn, value)


@functools.lru_cache(maxsize=None)
def _planes(H, W):
    """name -> plane: the designed planes and Bernoulli(p) planes at p = 0.1, 0.41 (near the 8-connected lattice's percolation
    threshold), 0.59 (near the 4-connected one's), 0.9"""
    out = dict(CR.designed(H, W))
    for p in (0.1, 0.41, 0.59, 0.9):
        out[f"bernoulli{p}"] = CR.bernoulli(H, W, p, int(p * 100) + H + 7 * W)
    return out


@functools.lru_cache(maxsize=None)
def _reference(H, W, conn, value):
    """(root [N, H, W], area [N, H, W], count [N]) of every plane of _planes(H, W): computed once, shared, never changed"""
    r = [_roots(m, conn, value) for m in _planes(H, W).values()]
    return np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.array([a[2] for a in r], dtype=np.int32)


def _stack(H, W):
    return torch.from_numpy(np.stack(list(_planes(H, W).values())))


def _eq(got, want):
    return got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


# ---- connected_components -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_connected_components_equals_scipy_bit_for_bit(H, W):
    """every designed and random plane, both connectivities, the set and the clear pixels, as one batch; then batches of 1, 3 and
    5 planes cut from other positions: a plane's outputs depend neither on P nor on its position"""
    from vdr import ops
    names = list(_planes(H, W))
    stack = _stack(H, W).to(DEV)
    N = stack.shape[0]
    for conn in (4, 8):
        for value in (0, 1):
            wr, wa, wc = _reference(H, W, conn, value)
            root, area, count = ops.connected_components(stack, conn, value)
            for k, name in enumerate(names):
                assert _eq(root[k], wr[k]) and _eq(area[k], wa[k]), (name, conn, value)
            assert _eq(count, wc)
            sel = (stack != 0) == bool(value)
            assert torch.equal(area.sum(dim=(1, 2)), sel.sum(dim=(1, 2)))                    # the areas sum to the selected pixels
            assert torch.equal((area != 0).sum(dim=(1, 2)).to(torch.int32), count)           # one nonzero area per component
            for P, s0 in ((1, 0), (1, N - 1), (3, 1), (3, N - 3), (5, 2), (5, N - 5)):
                r, a, c = ops.connected_components(stack[s0:s0 + P].bool() if P == 3 else stack[s0:s0 + P], conn, value)
                assert _eq(r, wr[s0:s0 + P]) and _eq(a, wa[s0:s0 + P]) and _eq(c, wc[s0:s0 + P]), (P, s0, conn, value)
    r, a, c = ops.connected_components(stack[N // 2], 8, 1)                                  # a 2-D mask: 2-D planes back
    assert tuple(r.shape) == (H, W) and _eq(r, _reference(H, W, 8, 1)[0][N // 2]) and tuple(c.shape) == (1,)


def test_designed_planes_have_the_components_they_were_designed_for():
    """the statements about the designs themselves, at 129 x 129 (four tiles and a fifth row and column of them)"""
    from vdr import ops
    H = W = 2 * T + 1
    pl = _planes(H, W)
    names = list(pl)
    stack = _stack(H, W).to(DEV)
    out = {c: ops.connected_components(stack, c, 1) for c in (4, 8)}
    cnt = {c: dict(zip(names, out[c][2].tolist())) for c in (4, 8)}
    assert cnt[4]["empty"] == cnt[8]["empty"] == 0 and cnt[4]["full"] == cnt[8]["full"] == 1 and cnt[4]["corners"] == cnt[8]["corners"] == 4
    assert cnt[8]["checkerboard"] == 1 and cnt[4]["checkerboard"] == (H * W) // 2             # one component at 8, one per pixel at 4
    assert cnt[8]["diagonal"] == cnt[8]["antidiagonal"] == 1 and cnt[4]["diagonal"] == cnt[4]["antidiagonal"] == H
    assert cnt[8]["corner_diag_main"] == cnt[8]["corner_diag_anti"] == 1 and cnt[4]["corner_diag_main"] == cnt[4]["corner_diag_anti"] == 2
    assert cnt[4]["serpentine"] == cnt[8]["serpentine"] == 1 and cnt[4]["comb"] == cnt[8]["comb"] == 1
    k = names.index("serpentine")
    root, area, _ = out[4]
    assert int(area[k, 0, 0]) == int(pl["serpentine"].sum()) and bool((root[k][stack[k] != 0] == 0).all())   # one chain across every seam
    k = names.index("corner_diag_anti")
    assert int(out[8][0][k, T, T - 1]) == (T - 1) * W + T and int(out[4][0][k, T, T - 1]) == T * W + T - 1
    assert cnt[4]["equal_areas"] == 3


def test_connected_components_memory_contract():
    """outputs and workspace of exactly the promised size between canaries; a workspace one byte short is VDR_ERR_WORKSPACE with
    the canary-filled outputs untouched"""
    from vdr import _lib
    lib = _lib.load()
    P, H, W = 3, T + 1, 2 * T + 1
    m = torch.from_numpy(np.stack([CR.bernoulli(H, W, p, 3) for p in (0.41, 0.59, 0.9)]))
    dev = m.to(DEV)
    need = lib.vdr_connected_components_workspace_bytes(P, H, W)
    assert need == 4 * P * H * W
    wr, root = mg.guarded(4 * P * H * W, 256)
    wa, area = mg.guarded(4 * P * H * W, 256)
    wc, count = mg.guarded(4 * P, 256)
    ww, work = mg.guarded(need, 256)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        return lib.vdr_op_connected_components(dev.data_ptr(), P, H, W, 4, 1, work.data_ptr(), nbytes, root.data_ptr(), area.data_ptr(), count.data_ptr(), stream)
    assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_connected_components: workspace too small")
    torch.cuda.synchronize()
    assert mg.canary_left(root.view(torch.int32)) == P * H * W and mg.canary_left(area.view(torch.int32)) == P * H * W
    assert mg.canary_left(count.view(torch.int32)) == P and mg.canary_left(work) == need
    assert call(need) == 0
    torch.cuda.synchronize()
    assert all(mg.guards_intact(w, 256) for w in (wr, wa, wc, ww))
    want = [_roots(m[p].numpy(), 4, 1) for p in range(P)]
    assert np.array_equal(root.view(torch.int32).reshape(P, H, W).cpu().numpy(), np.stack([w[0] for w in want]))
    assert np.array_equal(area.view(torch.int32).reshape(P, H, W).cpu().numpy(), np.stack([w[1] for w in want]))
    assert count.view(torch.int32).cpu().tolist() == [w[2] for w in want]


# ---- mask_clean ---------------------------------------------------------------------------------------------------------------------
CLEANS = (dict(min_area=9, holes=True, islands=True), dict(min_area=9, holes=True), dict(min_area=9, islands=True), dict(largest=True),
          dict(min_area=10 ** 6, islands=True), dict(min_area=30, holes=True, largest=True), dict())


@functools.lru_cache(maxsize=None)
def _clean_reference(H, W, conn, k):
    r = [CR.clean(m, connectivity=conn, roots=_roots, **CLEANS[k]) for m in _planes(H, W).values()]
    return np.stack([a[0] for a in r]), np.array([a[1] for a in r], dtype=np.int32), np.stack([a[2] for a in r])


@pytest.mark.parametrize("H,W", [(1, 1), (2, T), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (2 * T + 1, 2 * T + 1), (129, 257), (300, 517)])
def test_mask_clean_equals_the_restated_rules_bit_for_bit(H, W):
    from vdr import ops
    stack = _stack(H, W).to(DEV)
    N = stack.shape[0]
    for conn in (4, 8):
        for k, kw in enumerate(CLEANS):
            wo, wc, ws = _clean_reference(H, W, conn, k)
            out, changed, stats = ops.mask_clean(stack, connectivity=conn, **kw)
            assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), wo), (conn, kw)
            assert _eq(changed, wc) and _eq(stats, ws), (conn, kw)
            for P, s0 in ((1, N - 1), (3, 1), (5, N - 5)):
                o, c, s = ops.mask_clean(stack[s0:s0 + P], connectivity=conn, **kw)
                assert np.array_equal(o.cpu().numpy(), wo[s0:s0 + P]) and _eq(c, wc[s0:s0 + P]) and _eq(s, ws[s0:s0 + P]), (P, s0, conn, kw)
    o, c, s = ops.mask_clean(stack[0].bool(), largest=True)                                   # a 2-D bool mask
    assert tuple(o.shape) == (H, W) and tuple(c.shape) == (1,) and tuple(s.shape) == (1, 5)
    # results written into slices of larger tensors the caller owns: the same bits, nothing outside the slices touched
    big_o = torch.full((N + 2, H, W), 7, dtype=torch.uint8, device=DEV)
    big_c, big_s = torch.full((N + 2,), 7, dtype=torch.int32, device=DEV), torch.full((N + 2, 5), 7, dtype=torch.int32, device=DEV)
    wo, wc, ws = _clean_reference(H, W, 8, 0)
    ops.mask_clean(stack, connectivity=8, out=big_o[1:N + 1], changed=big_c[1:N + 1], stats=big_s[1:N + 1], **CLEANS[0])
    assert np.array_equal(big_o[1:N + 1].cpu().numpy(), wo) and _eq(big_c[1:N + 1], wc) and _eq(big_s[1:N + 1], ws)
    assert all(bool((t[0] == 7).all()) and bool((t[-1] == 7).all()) for t in (big_o, big_c, big_s))
    with pytest.raises(ValueError, match="mask_clean: out"):
        ops.mask_clean(stack, out=big_o)


def test_mask_clean_on_the_designs_made_for_it():
    """rings: a min_area between two hole areas fills some holes and not others; equal areas: the lowest root wins; every island
    below min_area: the largest stays; an empty plane and one with nothing to remove come back unchanged"""
    from vdr import ops
    H, W = T + 9, 2 * T + 1
    rings = CR.rings(H, W)
    _, area, n = _roots(rings, 8, 0)
    holes = np.sort(area[area > 0])
    assert n >= 4
    cut = int(holes[n // 2 - 1]) + 1                                                          # above the smaller half, at or below the rest
    assert holes[0] < cut <= holes[-1]
    out, changed, stats = ops.mask_clean(torch.from_numpy(rings).to(DEV), min_area=cut, holes=True)
    want = CR.clean(rings, min_area=cut, holes=True, roots=_roots)
    assert np.array_equal(out.cpu().numpy(), want[0]) and changed.tolist() == [1] and stats[0].tolist() == want[2].tolist()
    filled = int(out.sum()) - int(rings.sum())
    assert filled == int(holes[holes < cut].sum()) and 0 < filled < int(holes.sum())          # some holes filled, others left
    eq = CR.designed(H, W)["equal_areas"]
    stack = torch.from_numpy(np.stack([eq, np.zeros_like(eq), np.ones_like(eq)])).to(DEV)
    out, changed, stats = ops.mask_clean(stack, largest=True, connectivity=4)
    assert changed.tolist() == [2, 0, 0] and stats.tolist() == [[4, W - 2, 0, W - 1, 1], [0, 0, 0, 0, 0], [H * W, 0, 0, W - 1, H - 1]]
    out, changed, stats = ops.mask_clean(stack, min_area=100, islands=True, holes=True)        # every island below 100: the largest, lowest root
    assert changed.tolist() == [2, 0, 0] and stats[0].tolist() == [4, W - 2, 0, W - 1, 1]      # (the empty plane is one hole of H W >= 100 pixels: it stays)
    out, changed, stats = ops.mask_clean(stack, min_area=3, islands=True, holes=True)
    assert changed.tolist() == [2, 0, 0] and stats[0].tolist() == [8, 0, 0, W - 1, H - 1]      # only the single pixel goes


def test_mask_clean_reduces_more_than_64_chunks_a_plane():
    """513 x 513 is 65 chunks of 4096 pixels, the smallest square at which the finish kernel's loop over a plane's slots makes a
    second trip (lane 0 takes chunks 0 and 64).  Plane 0: 3 x 3 blobs in the first and the last corner and a single pixel at
    (y 512, x 0), so islands below 2 drops one pixel and the box spans the plane; plane 1: set pixels in chunk 64 alone, so its
    area and box come from the second trip only; plane 2: all clear.  Exact against vdr.components.clean_torch."""
    from vdr import components as cc
    from vdr import ops
    S = 513
    assert (S * S + 4095) // 4096 == 65 and 511 * S + 508 >= 64 * 4096
    m = torch.zeros((3, S, S), dtype=torch.uint8)
    m[0, :3, :3] = m[0, S - 3:, S - 3:] = 1
    m[0, 512, 0] = 1
    m[1, 511:513, 508:513] = 1
    for kw in (dict(min_area=2, islands=True), dict(largest=True)):
        wo, wc, ws = cc.clean_torch(m, **kw)
        out, changed, stats = ops.mask_clean(m.to(DEV), **kw)
        assert out.dtype == torch.uint8 and torch.equal(out.cpu(), wo) and _eq(changed, wc.numpy()) and _eq(stats, ws.numpy()), kw
        assert changed[2].item() == 0 and stats[2].tolist() == [0, 0, 0, 0, 0]                 # the all-clear plane
        if "islands" in kw:
            assert changed.tolist() == [2, 0, 0] and stats[:2].tolist() == [[18, 0, 0, 512, 512], [10, 508, 511, 512, 512]]
        else:
            assert changed.tolist() == [2, 0, 0] and stats[:2].tolist() == [[9, 0, 0, 2, 2], [10, 508, 511, 512, 512]]


def test_mask_clean_memory_contract():
    from vdr import _lib
    lib = _lib.load()
    P, H, W = 3, T + 1, 2 * T + 1
    m = torch.from_numpy(np.stack([CR.bernoulli(H, W, p, 5) for p in (0.41, 0.59, 0.9)]))
    dev = m.to(DEV)
    need = lib.vdr_mask_clean_workspace_bytes(P, H, W)
    chunks = (H * W + 4095) // 4096
    assert need == 8 * P * H * W + 8 * P + 8 * ((P + 1) // 2) + 2 * 32 * P * chunks
    wo, out = mg.guarded(P * H * W, 256)
    wc, changed = mg.guarded(4 * P, 256)
    ws, stats = mg.guarded(4 * 5 * P, 256)
    ww, work = mg.guarded(need, 256)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes, mode=3):
        return lib.vdr_op_mask_clean(dev.data_ptr(), P, H, W, 7, 8, mode, work.data_ptr(), nbytes, out.data_ptr(), changed.data_ptr(), stats.data_ptr(), stream)
    assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_mask_clean: workspace too small")
    torch.cuda.synchronize()
    assert mg.canary_left(out) == P * H * W and mg.canary_left(changed.view(torch.int32)) == P and mg.canary_left(stats.view(torch.int32)) == 5 * P
    assert mg.canary_left(work) == need
    assert call(need) == 0
    torch.cuda.synchronize()
    assert all(mg.guards_intact(w, 256) for w in (wo, wc, ws, ww))
    want = [CR.clean(m[p].numpy(), min_area=7, holes=True, islands=True, roots=_roots) for p in range(P)]
    assert np.array_equal(out.reshape(P, H, W).cpu().numpy(), np.stack([w[0] for w in want]))
    assert changed.view(torch.int32).cpu().tolist() == [w[1] for w in want]
    assert np.array_equal(stats.view(torch.int32).reshape(P, 5).cpu().numpy(), np.stack([w[2] for w in want]))
    assert lib.vdr_op_mask_clean(dev.data_ptr(), P, H, W, 7, 8, 3, work.data_ptr(), need, dev.data_ptr(), changed.data_ptr(), stats.data_ptr(), stream) == -1


# ---- mask_binarize ------------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("H,W,oh,ow", [(16, 16, 64, 64), (12, 20, 50, 75), (24, 24, 24, 24), (256, 256, 1024, 1024), (17, 3, 9, 2)])
def test_mask_binarize_is_the_upsampling_statement_and_mask_stats_pixels(H, W, oh, ow):
    """integer-valued and random logits at 4 x, at a non-integer scale, at the identity and at a down-sampling: bit for bit
    vdr.amg.upsample_torch > thr; its pixel count and box are mask_stats' n_mid and box on the same logits, read in place from
    a [P, 4, h, w] decode layout"""
    from vdr import amg, ops
    P = 3 if H < 256 else 1
    for kind, lg in (("integers", torch.randint(-3, 4, (P, 4, H, W), generator=torch.Generator().manual_seed(H + ow)).float()),
                     ("random", _randn((P, 4, H, W), 11 + H + oh, 2.0))):
        dev = lg.to(DEV)
        for thr in (0.0, 0.5, -1.25):
            want = (amg.upsample_torch(lg.reshape(-1, H, W), (oh, ow)) > thr).to(torch.uint8).reshape(P, 4, oh, ow)
            for view, w in ((dev[:, 2], want[:, 2]), (dev[:, 1:], want[:, 1:]), (dev.reshape(-1, H, W), want.reshape(-1, oh, ow))):
                got = ops.mask_binarize(view, (oh, ow), thr)
                assert got.dtype == torch.uint8 and torch.equal(got.cpu(), w), (kind, thr)
            got = ops.mask_binarize(dev[:, 1:], (oh, ow), thr)
            counts, box = ops.mask_stats(dev[:, 1:], (oh, ow), thr, 1.0)
            assert torch.equal(got.sum(dim=(2, 3)).to(torch.int32), counts[..., 1]), (kind, thr)
            _, _, stats = ops.mask_clean(got.reshape(-1, oh, ow))                             # mode 0: a copy and the statistics
            assert torch.equal(stats[:, 0], counts[..., 1].reshape(-1)) and torch.equal(stats[:, 1:], box.reshape(-1, 4)), (kind, thr)


# ---- the layers above: the tiny decoder geometry of tests/test_amg_gpu.py --------------------------------------------------------------
@pytest.fixture(scope="module")
def model(golden_dir):
    import amg_ref as AR
    import sam_prompt_ref as PR
    with AR.sam_model(PR.golden_prompts(golden_dir, "g8")[0], "sam_components_g8") as m:
        yield m


def _same_masks(got, logits_cpu, size, thr, **kw):
    """got = (masks, changed, stats) of a clean() call against clean_torch on the CPU up-sampling statement of the same logits"""
    from vdr import amg, components as cc
    lead = tuple(logits_cpu.shape[:-2])
    raw = amg.upsample_torch(logits_cpu.reshape(-1, *logits_cpu.shape[-2:]), size) > thr
    out, changed, stats = cc.clean_torch(raw, **kw)
    assert got[0].dtype == torch.bool and torch.equal(got[0].cpu(), out.bool().reshape(*lead, *size))
    assert torch.equal(got[1].cpu(), changed.reshape(lead)) and torch.equal(got[2].cpu(), stats.reshape(*lead, 5))
    return out.bool().reshape(*lead, *size), changed.reshape(lead)


def test_segmentation_clean_is_binarize_then_clean_torch(model):
    """Segmentation.clean on a three-mask decode and on the single-mask one (token 0 of the decode's four, read in place), at the
    input size and at another one, in chunks smaller than the batch; VolumeSegmentation.clean on a propagated volume"""
    m = model
    img = m.cfg.img
    x = _randn((2, 3, img, img), 5).to(DEV)
    boxes = torch.tensor([[[10.0, 12.0, 90.0, 100.0], [30.0, 20.0, 120.0, 70.0]]] * 2)
    changed_any = 0
    for multimask in (True, False):
        seg = m.segment(x, boxes, multimask=multimask)
        low = seg.low_res_logits.cpu()
        for size, thr, kw in (((img, img), 0.0, dict(min_area=25, holes=True, islands=True)), ((70, 93), 1.0, dict(min_area=0, holes=False, islands=False, largest=True)),
                              ((img, img), 2.0, dict(min_area=40, holes=True, islands=False, connectivity=4))):
            for max_planes in (64, 4):
                got = seg.clean(size=size, threshold=thr, max_planes=max_planes, **kw)
                _, changed = _same_masks(got, low, size, thr, **kw)
                changed_any |= int(changed.max())
        plain = seg.clean(min_area=0, holes=False, islands=False)                              # nothing asked: the masks themselves
        assert torch.equal(plain[0].cpu(), amg_masks(low, (img, img), 0.0)) and int(plain[1].abs().sum()) == 0
    assert changed_any == 3                                                                    # both steps did change some mask
    vol = m.propagate_masks(x[:1].expand(3, -1, -1, -1).contiguous(), boxes[0, 0], 1, max_batch=2)
    got = vol.clean(size=(50, 70), min_area=12)
    _same_masks(got, vol.low_res_logits.cpu(), (50, 70), 0.0, min_area=12, holes=True, islands=True)


def amg_masks(low_cpu, size, thr):
    from vdr import amg
    return (amg.upsample_torch(low_cpu.reshape(-1, *low_cpu.shape[-2:]), size) > thr).reshape(*low_cpu.shape[:-2], *size)


def test_pipeline_keywords_clean_the_volume_and_off_is_the_path_without_them(model):
    import vdr
    m = model
    H, W, S = 96, 80, 5
    vol = torch.rand((H, W, S), generator=torch.Generator().manual_seed(71)).numpy().astype(np.float32)
    box = np.array([20.0, 25.0, 60.0, 70.0])
    base = vdr.pipeline.segment_volume(m, vol, box, max_batch=2)
    off = vdr.pipeline.segment_volume(m, vol, box, max_batch=2, min_region_area=0, fill_holes=False, keep_largest=False)
    assert np.array_equal(base, off)
    # the path without the keywords, written out: prepare -> segment -> bilinear logits > threshold (what the parent computes)
    x = vdr.prep.prepare_slices(torch.from_numpy(vol).to(DEV)[:, :, 0:2], side=m.cfg.img, device=m.device)
    scaled = torch.tensor(box, dtype=torch.float64) * torch.tensor([m.cfg.img / W, m.cfg.img / H, m.cfg.img / W, m.cfg.img / H], dtype=torch.float64)
    seg = m.segment(x, scaled.reshape(1, 1, 4).expand(2, 1, 4))
    assert np.array_equal(base[:, :, 0:2], seg.masks(size=(H, W))[:, 0, 0].permute(1, 2, 0).cpu().numpy())
    low = seg.low_res_logits[:, 0, 0].cpu()
    for kw, ckw in ((dict(keep_largest=True), dict(largest=True)), (dict(min_region_area=30), dict(min_area=30, islands=True)),
                    (dict(min_region_area=30, fill_holes=True), dict(min_area=30, holes=True, islands=True)),
                    (dict(min_region_area=30, fill_holes=True, keep_largest=True), dict(min_area=30, holes=True, largest=True))):
        got = vdr.pipeline.segment_volume(m, vol, box, max_batch=2, **kw)
        assert got.shape == (H, W, S) and got.dtype == np.bool_
        from vdr import components as cc
        want = cc.clean_torch(amg_masks(low, (H, W), 0.0), **ckw)[0].bool()
        assert np.array_equal(got[:, :, 0:2], want.permute(1, 2, 0).numpy()), kw
    largest = vdr.pipeline.segment_volume(m, vol, box, max_batch=2, keep_largest=True)
    for s in range(S):                                                                       # one component a slice (or none)
        assert CR.roots_bfs(largest[:, :, s], 8, 1)[2] == min(1, int(base[:, :, s].any()))
    if not largest.any():                                                                    # (random weights: any mask will do for the plumbing)
        largest[30:50, 30:50, :] = True
    feats, masks = vdr.pipeline.generate_features(m, vol, largest)
    assert len(feats) == S and len(masks) == S and feats[0].shape[-1] == 256
    p0 = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2)
    assert np.array_equal(p0, vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2, min_region_area=0, fill_holes=False, keep_largest=False))
    p1 = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2, keep_largest=True)
    for s in range(S):
        assert np.array_equal(p1[:, :, s], CR.clean(p0[:, :, s], largest=True)[0].astype(bool)), s


def test_generate_masks_small_region_removal_is_the_rule_restated_on_the_host(model):
    """min_mask_region_area = 0 is the call without the keyword in every field; a positive area is segment_anything's
    postprocess_small_regions restated from that result: binarise, holes then islands at 8-connectivity, boxes of the cleaned
    masks, a second NMS with score 1 for an unchanged mask and 0 for a changed one, survivors in rank order"""
    from vdr import amg
    m = model
    img = m.cfg.img
    x = _randn((1, 3, img, img), 5).to(DEV)
    tested = 0
    for mask_thr, nms_thr in ((3.0, 0.9), (3.5, 0.97), (0.0, 0.7)):
        kw = dict(points_per_side=4, pred_iou_thresh=-1.0e30, stability_score_thresh=0.0, mask_threshold=mask_thr, box_nms_thresh=nms_thr)
        ms0 = m.generate_masks(x, **kw)
        same = m.generate_masks(x, min_mask_region_area=0, **kw)
        assert same.cleaned is None and same.changed is None and len(same) == len(ms0)
        for f in ("low_res_logits", "iou", "stability", "area", "boxes", "points", "point_index", "mask_index"):
            assert torch.equal(getattr(same, f), getattr(ms0, f)), f
        K = len(ms0)
        if K == 0:
            continue
        raw = (amg.upsample_torch(ms0.low_res_logits.cpu(), (img, img)) > mask_thr).numpy()
        for area in (20, 300):
            cleaned = [CR.clean(raw[k], min_area=area, holes=True, islands=True, connectivity=8, roots=_roots) for k in range(K)]
            out = np.stack([c[0] for c in cleaned])
            changed = torch.tensor([c[1] for c in cleaned], dtype=torch.int32)
            stats = torch.from_numpy(np.stack([c[2] for c in cleaned]))
            kept, count = amg.nms_torch(stats[:, 1:].float(), (changed == 0).float(), nms_thr)
            keep = torch.sort(kept[:int(count)].long()).values
            ms = m.generate_masks(x, min_mask_region_area=area, **kw)
            assert len(ms) == keep.numel() and ms.cleaned.dtype == torch.uint8 and tuple(ms.cleaned.shape) == (keep.numel(), img, img)
            assert np.array_equal(ms.cleaned.cpu().numpy(), out[keep.numpy()]) and torch.equal(ms.changed.cpu(), changed[keep])
            assert torch.equal(ms.area.cpu(), stats[keep, 0]) and torch.equal(ms.boxes.cpu(), stats[keep, 1:])
            for f in ("low_res_logits", "iou", "stability", "points", "point_index", "mask_index"):
                assert torch.equal(getattr(ms, f).cpu(), getattr(ms0, f).cpu()[keep]), f
            assert torch.equal(ms.masks().cpu(), torch.from_numpy(out[keep.numpy()]).bool()) and len(ms.rle()) == len(ms)
            assert int(ms.label_map().max()) <= len(ms)
            with pytest.raises(ValueError, match="cleaned"):
                ms.masks((img // 2, img // 2))
            tested += int(changed.any())
            print(f"mask_threshold {mask_thr} nms {nms_thr} area {area}: {K} masks, {int((changed != 0).sum())} changed, {keep.numel()} kept")
    assert tested >= 2                                                                       # the rule did change masks


def test_device_labelling_of_tokencut_and_lost_equals_the_host_one():
    """designed bipartitions (a grid below a tile and one across four tiles), then LOST and TokenCut on a golden graph and on the
    tiny model, labelling="device" against "host" in every field"""
    import handle_configs as hc
    from oracle import vit_oracle as vo
    from spectral_ref import load_golden
    from vdr import ops, spectral
    for gh, gw in ((10, 13), (T + 6, T + 3)):
        parts, seeds = [], []
        for name, pl in CR.designed(gh, gw).items():
            if pl.any():
                parts.append(pl.reshape(-1).astype(bool))
                seeds.append(int(np.flatnonzero(pl.reshape(-1))[-1]))                         # the last set pixel: far from the root
        parts.append(CR.bernoulli(gh, gw, 0.59, 4).reshape(-1).astype(bool))
        seeds.append(int(np.flatnonzero(parts[-1])[len(np.flatnonzero(parts[-1])) // 2]))
        host = spectral._masks_and_boxes(parts, seeds, (gh, gw), DEV)
        dev = spectral._masks_and_boxes_device(parts, seeds, (gh, gw), DEV)
        for a, b in zip(host, dev):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (gh, gw)
    g, t, _, x = load_golden("333x96")
    bits = ops.affinity_bits(x[None].cuda().expand(2, -1, -1), tau=0.0)
    grid = tuple(g["grid"])

    def same(a, b, fields):
        for f in fields:
            u, v = getattr(a, f), getattr(b, f)
            assert (torch.equal(u, v) and u.dtype == v.dtype) if isinstance(u, torch.Tensor) else u == v, f
    lost_fields = ("degree", "expansion", "seed", "mask", "box", "grid", "stride", "patch", "bits")
    cut_fields = ("eigvec", "bipartition", "seed", "mask", "box", "grid", "stride", "patch", "eigval", "resid", "steps", "bits")
    for k in (1, 40, 1000):
        same(spectral.lost(bits, grid, k=k, labelling="device"), spectral.lost(bits, grid, k=k), lost_fields)
    bits = ops.affinity_bits(x[None].cuda(), tau=float(g["tau"]))
    same(spectral.tokencut(bits, grid, eps=float(g["eps"]), labelling="device"), spectral.tokencut(bits, grid, eps=float(g["eps"])), cut_fields)
    with hc.registered_model("_components_tiny") as tiny:
        images = vo.make_images(hc.TINY, 3, seed=6).cuda()
        tiny.set_patch_stride(4)                                                             # a 7 x 7 grid
        try:
            same(tiny.tokencut(images, tau=0.8, labelling="device"), tiny.tokencut(images, tau=0.8), cut_fields)
            same(tiny.lost(images, k=5, tau=0.8, labelling="device"), tiny.lost(images, k=5, tau=0.8), lost_fields)
        finally:
            tiny.set_patch_stride(8)
        with pytest.raises(ValueError, match="labelling"):
            tiny.tokencut(images, labelling="gpu")
