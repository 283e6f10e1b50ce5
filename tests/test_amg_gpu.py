"""GPU: the automatic mask generator -- vdr_op_mask_stats and vdr_op_nms bit for bit against their torch statements
(vdr.amg.mask_stats_torch / nms_torch: the same arithmetic, no tolerance), their memory contract (canaries, a workspace one byte
short), model.generate_masks bit for bit against the composition decode_masks + mask_stats_torch + nms_torch written out here,
and the scoring against transformers' golden inside the gates of tests/golden/README_amg.md.  Nothing is derived from device
output."""
import pytest
import torch

import amg_ref as AR
import memguard as mg
import sam_prompt_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
THRESHOLDS = ((0.0, 1.0), (0.5, 0.0), (-0.25, 0.75))   # (threshold, offset); the second: off = 0, the three counts coincide


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _same(got, want):
    return got.dtype == want.dtype and torch.equal(got.cpu(), want)


# ---- mask_stats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,oh,ow,P", [(1, 1, 3, 5, 3), (8, 8, 32, 32, 130), (12, 20, 50, 75, 130), (17, 3, 9, 2, 3), (64, 64, 256, 256, 3),
                                         (256, 256, 1024, 1024, 1)])
def test_mask_stats_equals_its_torch_statement_bit_for_bit(H, W, oh, ow, P):
    """random fp32 logits as [P, 4, H, W]: one token read in place (strided planes), tokens 1 .. 3 in place (groups of three), and
    the dense copy; P planes and the first plane alone (P = 1).  The references are computed once, on the CPU."""
    from vdr import amg, ops
    lg = _randn((P, 4, H, W), 100 + H + oh, 3.0)
    dev = lg.to(DEV)
    for thr, off in THRESHOLDS:
        want_c, want_b = amg.mask_stats_torch(lg.reshape(-1, H, W), (oh, ow), thr, off)
        want_c, want_b = want_c.reshape(P, 4, 3), want_b.reshape(P, 4, 4)
        for t in (0, 3):                                                                     # a token plane of [P, 4, H, W], in place
            view = dev[:, t]
            assert not view.is_contiguous() or P == 1
            c, b = ops.mask_stats(view, (oh, ow), thr, off)
            assert tuple(c.shape) == (P, 3) and tuple(b.shape) == (P, 4)
            assert _same(c, want_c[:, t]) and _same(b, want_b[:, t]), (thr, off, t)
        c, b = ops.mask_stats(dev[:, 1:], (oh, ow), thr, off)                                # tokens 1 .. 3: [P, 3, H, W] in place
        assert tuple(c.shape) == (P, 3, 3) and _same(c, want_c[:, 1:]) and _same(b, want_b[:, 1:]), (thr, off)
        c, b = ops.mask_stats(dev.reshape(-1, H, W), (oh, ow), thr, off)                     # dense
        assert _same(c, want_c.reshape(-1, 3)) and _same(b, want_b.reshape(-1, 4)), (thr, off)
        if off == 0.0:
            assert bool((c[:, 0] == c[:, 1]).all()) and bool((c[:, 1] == c[:, 2]).all())
    # a plane's result alone is its result inside the batch, wherever it stands
    thr, off = THRESHOLDS[-1]                                                                # (want_c, want_b: the last pair's)
    cb, bb = ops.mask_stats(dev[:, 2], (oh, ow), thr, off)
    for p in sorted({0, P // 2, P - 1}):
        c1, b1 = ops.mask_stats(dev[p:p + 1, 2], (oh, ow), thr, off)
        assert _same(c1, want_c[p:p + 1, 2]) and _same(b1, want_b[p:p + 1, 2])
        assert torch.equal(c1[0], cb[p]) and torch.equal(b1[0], bb[p])


@pytest.mark.parametrize("H,W,oh,ow", [(8, 8, 32, 32), (12, 20, 50, 75), (17, 3, 9, 2), (5, 7, 4096, 33)])
def test_mask_stats_on_designed_planes(H, W, oh, ow):
    """an all-negative plane (empty box, n_lo = 0), an all-positive one, and a single positive source pixel in each corner and in
    the middle of the last row and column (where y1 = y0 and x1 = x0 clamp)"""
    from vdr import amg, ops
    lg = torch.full((9, H, W), -2.0)
    lg[1] = 2.0
    for p, (y, x) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, W // 2), (H // 2, W - 1), (H // 2, W // 2)], start=2):
        lg[p, y, x] = 5.0
    for thr, off in THRESHOLDS:
        want_c, want_b = amg.mask_stats_torch(lg, (oh, ow), thr, off)
        c, b = ops.mask_stats(lg.to(DEV), (oh, ow), thr, off)
        assert _same(c, want_c) and _same(b, want_b), (thr, off)
    c, b = ops.mask_stats(lg.to(DEV), (oh, ow), 0.0, 1.0)
    assert c[0].tolist() == [0, 0, 0] and b[0].tolist() == [0, 0, 0, 0]                      # empty: transformers' 0, 0, 0, 0
    assert c[1].tolist() == [oh * ow] * 3 and b[1].tolist() == [0, 0, ow - 1, oh - 1]
    assert b[2, :2].tolist() == [0, 0] and b[5, 2:].tolist() == [ow - 1, oh - 1]            # the corners reach the image's corners
    assert bool(amg.stability(c)[0].isnan())


def test_mask_stats_reduces_128_bands_from_the_last_one():
    """(5, 7) -> (4096, 33) is 128 bands a plane, two trips of the finish kernel's loop over the slots.  Plane 0: only the last source
    pixel is above the threshold, so every count and the box's minima and maxima come from the last bands and the last columns while
    all other slots hold the identity; plane 1: everything below, box 0, 0, 0, 0.  Exact against vdr.amg.mask_stats_torch."""
    from vdr import amg, ops
    H, W, oh, ow = 5, 7, 4096, 33
    lg = torch.full((2, H, W), -2.0)
    lg[0, H - 1, W - 1] = 5.0
    for thr, off in THRESHOLDS:
        want_c, want_b = amg.mask_stats_torch(lg, (oh, ow), thr, off)
        c, b = ops.mask_stats(lg.to(DEV), (oh, ow), thr, off)
        assert _same(c, want_c) and _same(b, want_b), (thr, off)
        x0, y0, x1, y1 = b[0].tolist()
        assert c[0, 1].item() > 0 and (x1, y1) == (ow - 1, oh - 1) and y0 > oh - 2 * oh // H and x0 > ow - 2 * ow // W   # inside the last source pixel's reach
        assert c[1].tolist() == [0, 0, 0] and b[1].tolist() == [0, 0, 0, 0]


def test_mask_stats_memory_contract():
    """outputs and workspace of exactly the promised size between canaries; a workspace one byte short is VDR_ERR_WORKSPACE with
    nothing written"""
    from vdr import _lib, amg
    lib = _lib.load()
    P, H, W, oh, ow = 5, 12, 20, 100, 75
    lg = _randn((P, H, W), 7, 3.0)
    dev = lg.to(DEV)
    need = lib.vdr_mask_stats_workspace_bytes(P, H, W, oh, ow)
    assert need == P * 4 * 32                                                               # 4 bands of 32 rows, 32 bytes a slot
    wc, counts = mg.guarded(P * 3 * 4, 256)
    wb, box = mg.guarded(P * 4 * 4, 256)
    ww, work = mg.guarded(need, 256)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        return lib.vdr_op_mask_stats(dev.data_ptr(), H * W, P, 0, P, H, W, oh, ow, 0.0, 1.0, work.data_ptr(), nbytes, counts.data_ptr(), box.data_ptr(), stream)
    assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_mask_stats: workspace too small")
    torch.cuda.synchronize()
    assert mg.canary_left(counts.view(torch.int32)) == P * 3 and mg.canary_left(box.view(torch.int32)) == P * 4 and mg.canary_left(work) == need
    assert call(need) == 0
    torch.cuda.synchronize()
    assert mg.guards_intact(wc, 256) and mg.guards_intact(wb, 256) and mg.guards_intact(ww, 256)
    want_c, want_b = amg.mask_stats_torch(lg, (oh, ow), 0.0, 1.0)
    assert torch.equal(counts.view(torch.int32).reshape(P, 3).cpu(), want_c) and torch.equal(box.view(torch.int32).reshape(P, 4).cpu(), want_b)


# ---- nms ------------------------------------------------------------------------------------------------------------------------
def test_nms_on_designed_boxes():
    from vdr import ops
    for name, (boxes, scores, thr, want) in AR.designed_boxes().items():
        kept, count = ops.nms(boxes.to(DEV), scores.to(DEV), thr)
        assert kept.dtype == torch.int32 and count.dtype == torch.int32 and int(count) == len(want), name
        assert kept.tolist() == want + [-1] * (boxes.shape[0] - len(want)), name


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 129, 1000, 4096])
def test_nms_equals_its_torch_statement_bit_for_bit(N):
    """random boxes with heavy overlap, zero-area boxes, copies and many equal scores; all-disjoint boxes (nothing goes: the walk's
    longest chain); two runs bitwise equal"""
    from vdr import amg, ops
    boxes, scores = AR.random_boxes(N, 30 + N)
    for thr in (0.5, 0.1):
        want_kept, want_count = amg.nms_torch(boxes, scores, thr)
        kept, count = ops.nms(boxes.to(DEV), scores.to(DEV), thr)
        again = ops.nms(boxes.to(DEV), scores.to(DEV), thr)
        assert _same(count, want_count) and _same(kept, want_kept), (N, thr)
        assert torch.equal(again[0], kept) and torch.equal(again[1], count)
        if N >= 63:
            assert 1 <= int(count) < N                                                          # the sets do suppress
    boxes, scores = AR.disjoint_boxes(N)
    kept, count = ops.nms(boxes.to(DEV), scores.to(DEV), 0.7)
    assert int(count) == N and kept.tolist() == list(range(N))


def test_nms_memory_contract():
    from vdr import _lib, amg
    lib = _lib.load()
    N = 130
    boxes, scores = AR.random_boxes(N, 9)
    order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32).to(DEV)
    bx = boxes.to(DEV)
    need = lib.vdr_nms_workspace_bytes(N)
    assert need == N * 3 * 8
    wk, keep = mg.guarded(N, 256)
    wl, kept = mg.guarded(N * 4, 256)
    wn, count = mg.guarded(4, 256)
    ww, work = mg.guarded(need, 256)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        return lib.vdr_op_nms(bx.data_ptr(), order.data_ptr(), N, 0.5, work.data_ptr(), nbytes, keep.data_ptr(), kept.data_ptr(), count.data_ptr(), stream)
    assert call(need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_nms: workspace too small")
    torch.cuda.synchronize()
    assert mg.canary_left(keep) == N and mg.canary_left(kept.view(torch.int32)) == N and mg.canary_left(count.view(torch.int32)) == 1
    assert call(need) == 0
    torch.cuda.synchronize()
    assert all(mg.guards_intact(w, 256) for w in (wk, wl, wn, ww))
    want_kept, want_count = amg.nms_torch(boxes, scores, 0.5)
    assert torch.equal(kept.view(torch.int32).cpu(), want_kept) and torch.equal(count.view(torch.int32).cpu(), want_count)
    flags = torch.zeros(N, dtype=torch.uint8)
    flags[want_kept[:int(want_count)].long()] = 1
    assert torch.equal(keep.cpu(), flags)                                                       # every flag written: 1 kept, 0 suppressed


# ---- generate_masks ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(golden_dir):
    return PR.golden_prompts(golden_dir, "g8")[0]


@pytest.fixture(scope="module")
def model(base):
    with AR.sam_model(base, "sam_amg_g8") as m:
        yield m


CONFIGS = ((0.0, 0.7), (3.0, 0.9), (3.0, 0.95), (4.0, 0.9), (3.5, 0.97))   # (mask_threshold, box_nms_thresh)


@pytest.fixture(scope="module")
def composed(model):
    """decode_masks + mask_stats_torch + nms_torch on a seeded image, step by step, for every configuration of CONFIGS.  The
    miniature's masks are noise that spans most of the image, so at SAM's defaults NMS keeps one box: the further configurations
    raise the mask threshold until the boxes differ.  The filter thresholds are quantiles of the composition's own candidates,
    so that both filters cut; at least one configuration must keep several masks AND suppress some."""
    from vdr import amg
    m = model
    img, g4 = m.cfg.img, 4 * m.mask_decoder.g
    x = _randn((1, 3, img, img), 5).to(DEV)
    grid = amg.point_grid(4, img)
    n = grid.shape[0]
    seg = m.decode_masks(m.image_encoder(x), points=grid.reshape(1, n, 1, 2), point_labels=torch.ones((1, n, 1), dtype=torch.int32), multimask=True)
    low, iou = seg.low_res_logits[0].reshape(n * 3, g4, g4).cpu(), seg.iou[0].reshape(-1).cpu()
    out = []
    for mask_thr, nms_thr in CONFIGS:
        counts, box = amg.mask_stats_torch(low, (img, img), mask_thr, 1.0)
        stab = amg.stability(counts)
        finite = stab[~stab.isnan()]
        t_iou, t_stab = float(iou.quantile(0.3)), float(finite.quantile(0.25)) if finite.numel() else 0.0
        cand = ((iou > t_iou) & (stab > t_stab)).nonzero()[:, 0]
        sel = cand
        if cand.numel():
            kept, count = amg.nms_torch(box[cand].float(), iou[cand], nms_thr)
            sel = cand[kept[:int(count)].long()]
        print(f"mask_threshold {mask_thr} nms {nms_thr}: {cand.numel()} of {n * 3} candidates pass, {sel.numel()} kept")
        out.append(dict(x=x, grid=grid, low=low, iou=iou, counts=counts, box=box, stab=stab, sel=sel, cand=int(cand.numel()), kw=dict(
            points_per_side=4, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, stability_score_offset=1.0, mask_threshold=mask_thr, box_nms_thresh=nms_thr)))
    assert any(2 <= c["sel"].numel() < c["cand"] for c in out)
    return out


def _check(ms, c):
    sel = c["sel"]
    assert len(ms) == sel.numel()
    assert _same(ms.low_res_logits, c["low"][sel]) and _same(ms.iou, c["iou"][sel]) and _same(ms.stability, c["stab"][sel])
    assert _same(ms.area, c["counts"][sel, 1]) and _same(ms.boxes, c["box"][sel]) and _same(ms.points, c["grid"][sel // 3])
    assert ms.point_index.cpu().tolist() == (sel // 3).tolist() and ms.mask_index.cpu().tolist() == (sel % 3).tolist()


def test_generate_masks_is_the_composition_bit_for_bit(model, composed):
    for c in composed:
        ms = model.generate_masks(c["x"], points_per_batch=64, **c["kw"])
        _check(ms, c)
        K = len(ms)
        assert bool((ms.iou[1:] <= ms.iou[:-1]).all())                                          # NMS order: best predicted IoU first
        if K == 0:
            continue
        # the stored logits are a direct decode of the stored points, bit for bit
        seg = model.decode_masks(model.image_encoder(c["x"]), points=ms.points.reshape(1, K, 1, 2), point_labels=torch.ones((1, K, 1), dtype=torch.int32),
                                 multimask=True)
        direct = seg.low_res_logits[0][torch.arange(K, device=DEV), ms.mask_index]
        assert torch.equal(direct, ms.low_res_logits)
        # the methods agree with the stored statistics
        masks = ms.masks()
        assert masks.dtype == torch.bool and tuple(masks.shape) == (K, model.cfg.img, model.cfg.img)
        lm = ms.label_map()
        assert lm.dtype == torch.int32 and int(lm.max()) <= K and len(ms.rle()) == K
        assert ms.boxes_xywh()[:, 2].tolist() == (ms.boxes[:, 2] - ms.boxes[:, 0]).tolist()


def test_generate_masks_does_not_depend_on_the_batch_size(model, composed):
    for c in composed:
        _check(model.generate_masks(c["x"], points_per_batch=4, **c["kw"]), c)
        _check(model.generate_masks(c["x"][0], points_per_batch=5, **c["kw"]), c)              # [3, S, S]; a ragged last batch


def test_generate_masks_with_thresholds_that_keep_nothing_is_empty(model, composed):
    kw = dict(composed[0]["kw"], pred_iou_thresh=1e9)
    ms = model.generate_masks(composed[0]["x"], **kw)
    g4 = 4 * model.mask_decoder.g
    assert len(ms) == 0 and tuple(ms.low_res_logits.shape) == (0, g4, g4) and tuple(ms.boxes.shape) == (0, 4) and tuple(ms.points.shape) == (0, 2)
    assert tuple(ms.masks().shape) == (0, model.cfg.img, model.cfg.img) and int(ms.label_map().sum()) == 0 and ms.rle() == []


def test_scores_stay_inside_the_gates_of_the_transformers_golden(model, base, golden_dir):
    """fp32 SamModel against the bf16 library on the golden's embedding: per candidate the stability score, the area and the
    predicted IoU within 2 x the CPU-measured difference of the bf16 restatement; the filter decision equal for every candidate
    that is further from both thresholds than those gates (the generator asserts that this leaves out at most a quarter)"""
    g = AR.golden_amg(golden_dir)
    img, n = model.cfg.img, g["grid"].shape[0]
    seg = model.decode_masks(base["emb"][:1].to(DEV), points=g["grid"].reshape(1, n, 1, 2), point_labels=torch.ones((1, n, 1), dtype=torch.int32), multimask=True)
    counts, box, stab = seg.stats((img, img), 0.0, g["offset"])
    counts, stab, iou = counts[0].cpu(), stab[0].cpu(), seg.iou[0].cpu()
    both = ~(stab.isnan() | g["stability"].isnan())
    d_stab = float((stab - g["stability"])[both].abs().max())
    d_area = int((counts[..., 1] - g["counts"][..., 1]).abs().max())
    d_iou = float((iou - g["iou"]).abs().max())
    print(f"stability {d_stab:.3e} (gate {g['gate_stability']:.3e})  area {d_area} px (gate {g['gate_area']})  iou {d_iou:.3e} (gate {g['gate_iou']:.3e})")
    assert torch.equal(stab.isnan(), g["stability"].isnan())
    assert d_stab <= g["gate_stability"] and d_area <= g["gate_area"] and d_iou <= g["gate_iou"]
    keep = (iou > g["pred_iou_thresh"]) & (stab > g["stability_score_thresh"])
    clear = g["clear"]
    assert float((~clear).double().mean()) <= 0.25 and bool((g["keep"] & clear).any()) and bool((~g["keep"] & clear).any())
    assert torch.equal(keep[clear], g["keep"][clear])
