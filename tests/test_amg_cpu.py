"""CPU: the automatic mask generator without a device -- the torch statements of the two kernels (vdr.amg.mask_stats_torch,
nms_torch) against F.interpolate, a float64 brute force, transformers' helpers (tests/golden/README_amg.md) and designed boxes;
point_grid and rle against transformers' stored output; every refusal of generate_masks and of the two C entry points before
the device is touched; the mapping of the statistics kernel walked by a host program, plainly and under the sanitizers."""
import ctypes as C
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import amg_ref as AR
import host_program

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")
EPS = float(torch.finfo(torch.float32).eps)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _hf_box(mask):
    """transformers' _batched_mask_to_box on one [h, w] bool mask, restated with any / nonzero"""
    if not bool(mask.any()):
        return [0, 0, 0, 0]
    ys, xs = mask.any(dim=1).nonzero()[:, 0], mask.any(dim=0).nonzero()[:, 0]
    return [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])]


# ---- mask_stats_torch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,oh", [(8, 32), (32, 128)])
def test_torch_statement_is_interpolate_bit_for_bit_on_integer_logits_at_4x(H, oh):
    """integer-valued logits, weights that are multiples of 1/8: every product and sum is exact, so any order gives the same bits"""
    from vdr import amg
    x = torch.randint(-8, 9, (5, H, H), generator=torch.Generator().manual_seed(H)).float()
    x[3], x[4] = -3.0, 2.0                                                          # an empty and a full plane
    ref = F.interpolate(x[:, None], size=(oh, oh), mode="bilinear", align_corners=False)[:, 0]
    assert torch.equal(amg.upsample_torch(x, (oh, oh)).view(torch.int32), ref.view(torch.int32))
    for thr, off in ((0.0, 1.0), (0.5, 0.25), (-1.0, 0.0)):
        counts, box = amg.mask_stats_torch(x, (oh, oh), thr, off)
        assert counts.dtype == torch.int32 and box.dtype == torch.int32
        for p in range(5):
            want = [int((ref[p] > thr + off).sum()), int((ref[p] > thr).sum()), int((ref[p] > thr - off).sum())]
            assert counts[p].tolist() == want and box[p].tolist() == _hf_box(ref[p] > thr), (p, thr, off)
    counts, box = amg.mask_stats_torch(x, (oh, oh))
    assert counts[3].tolist() == [0, 0, 0] and box[3].tolist() == [0, 0, 0, 0]
    assert counts[4].tolist() == [oh * oh] * 3 and box[4].tolist() == [0, 0, oh - 1, oh - 1]
    assert bool(amg.stability(counts)[3].isnan()) and float(amg.stability(counts)[4]) == 1.0


@pytest.mark.parametrize("shape", [(24, 40, 100, 150), (32, 32, 100, 100)])
def test_torch_statement_on_random_logits_differs_from_interpolate_only_at_the_thresholds(shape):
    """Non-dyadic scales: ATen's kernel and the stated formula round differently, so a pixel whose value is a threshold's to
    within 4 eps max|logit| may fall on either side.  The counts may differ by at most the number of such reference pixels,
    the box by nothing unless such a pixel lies on its edge.  The float64 brute force bounds the statement's own error."""
    from vdr import amg
    H, W, oh, ow = shape
    x = _randn((4, H, W), 3 + H, 4.0)
    ref = F.interpolate(x[:, None], size=(oh, ow), mode="bilinear", align_corners=False)[:, 0]
    mine = amg.upsample_torch(x, (oh, ow))
    dist = 4.0 * EPS * float(x.abs().max())
    exact = AR.upsample_f64(x, (oh, ow))
    # the statement against the definition: the source coordinate's fp32 error (a few eps of H) times the slope, plus the blend's roundings
    slope = float(max((x[:, 1:] - x[:, :-1]).abs().max(), (x[:, :, 1:] - x[:, :, :-1]).abs().max()))
    own = 8.0 * EPS * max(H, W) * slope + 4.0 * EPS * float(x.abs().max())
    print(f"{shape}: max|statement - interpolate| {float((mine - ref).abs().max()):.3e}, max|statement - float64| {float((mine - exact).abs().max()):.3e} "
          f"(bound {own:.3e}), window {dist:.3e}")
    assert float((mine - exact).abs().max()) <= own
    thr, off = 0.0, 1.0
    counts, box = amg.mask_stats_torch(x, (oh, ow), thr, off)
    for k, t in enumerate((thr + off, thr, thr - off)):
        want, slack = (ref > t).sum((-1, -2)), AR.near(ref, t, dist)
        print(f"  threshold {t}: counts {counts[:, k].tolist()} interpolate {want.tolist()} pixels in the window {slack.tolist()}")
        assert bool(((counts[:, k] - want).abs() <= slack).all())
    edge = ((ref - thr).abs() <= dist)
    for p in range(4):
        want = _hf_box(ref[p] > thr)
        if box[p].tolist() != want:   # only a window pixel on the box's edge may move it
            ys, xs = edge[p].nonzero()[:, 0].tolist(), edge[p].nonzero()[:, 1].tolist()
            assert any(x_ in (want[0], want[2], box[p, 0], box[p, 2]) or y_ in (want[1], want[3], box[p, 1], box[p, 3]) for y_, x_ in zip(ys, xs))


def test_statement_reproduces_transformers_scores_and_boxes(golden_dir):
    """the stored output of _compute_stability_score / _batched_mask_to_box on SamModel's masks (F.interpolate to the image
    size): a 4 x up-sampling of non-integer logits -- dyadic weights, but products that round -- so the rule of the test above
    applies: counts inside the window count, boxes equal unless a window pixel lies on an edge"""
    from vdr import amg
    g = AR.golden_amg(golden_dir)
    low = g["low_res"]
    n, S = low.shape[0], 4 * low.shape[-1]
    planes = low.reshape(-1, *low.shape[-2:])
    counts, box = amg.mask_stats_torch(planes, (S, S), 0.0, g["offset"])
    ref = F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False).reshape(-1, S, S)
    dist = 4.0 * EPS * float(low.abs().max())
    want = g["counts"].reshape(-1, 3)
    for k, t in enumerate((g["offset"], 0.0, -g["offset"])):
        assert bool(((counts[:, k] - want[:, k]).abs() <= AR.near(ref, t, dist)).all())
    print(f"golden: {int((counts != want).sum())} of {counts.numel()} counts differ from transformers'; window {dist:.3e}")
    clean = AR.near(ref, 0.0, dist) == 0
    assert int(clean.sum()) >= planes.shape[0] // 2 and torch.equal(box[clean], g["boxes"].reshape(-1, 4)[clean])
    same = (counts == want).all(dim=1)
    st, ref_st = amg.stability(counts).reshape(n, 3), g["stability"]
    assert torch.equal(st.isnan(), ref_st.isnan())
    assert torch.equal(st.reshape(-1)[same].view(torch.int32), ref_st.reshape(-1)[same].view(torch.int32))   # int / int in fp32: the same division


def test_point_grid_and_rle_are_transformers(golden_dir):
    from vdr import amg
    g = AR.golden_amg(golden_dir)
    grid = amg.point_grid(g["n_per_side"], 128)
    assert grid.dtype == torch.float32 and torch.equal(grid, g["grid"])
    assert grid[1].tolist() == [48.0, 16.0]                                          # x runs fastest
    assert amg.point_grid(1, 1024).tolist() == [[512.0, 512.0]]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_per_side"):
            amg.point_grid(bad, 128)
    rle = amg.mask_to_rle(g["rle_masks"])
    assert [r["counts"] for r in rle] == g["rle"] and all(r["size"] == [6, 5] for r in rle)
    assert rle[0]["counts"] == [30] and rle[1]["counts"] == [0, 30] and rle[2]["counts"][:2] == [0, 1]   # empty, full, first pixel set


# ---- nms_torch ------------------------------------------------------------------------------------------------------------------
def test_nms_statement_on_designed_boxes():
    from vdr import amg
    for name, (boxes, scores, thr, want) in AR.designed_boxes().items():
        kept, count = amg.nms_torch(boxes, scores, thr)
        assert kept.dtype == torch.int32 and int(count) == len(want), name
        assert kept.tolist() == want + [-1] * (boxes.shape[0] - len(want)), name
    boxes, scores = AR.disjoint_boxes(130)
    assert amg.nms_torch(boxes, scores, 0.7)[0].tolist() == list(range(130))
    boxes, scores = AR.random_boxes(300, 5)
    kept, count = amg.nms_torch(boxes, scores, 0.3)
    k = kept[:int(count)].long()
    assert 1 < int(count) < 300 and bool((kept[int(count):] == -1).all()) and bool((scores[k][1:] <= scores[k][:-1]).all())


# ---- the C side -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_listed_in_the_makefile():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    lib = _lib.load()
    for name in ("vdr_op_mask_stats", "vdr_op_nms"):
        assert re.search(r"\bint " + name + r"\(", src) and name in _lib.SYMBOLS and hasattr(lib, name), name
    for name in ("vdr_mask_stats_workspace_bytes", "vdr_nms_workspace_bytes"):
        assert re.search(r"\bsize_t " + name + r"\(", src) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.vdr_abi_version() == 8 and "#define VDR_ABI_VERSION 8" in src               # additive: the version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for unit in ("mask_stats", "nms"):
        assert re.search(r"^NOCONTRACT :=.*\b" + unit + r"\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\b" + unit + r"\.hip\b", mk, re.M)
        assert re.search(r"^ASM :=.*\b" + unit + r"\b", mk, re.M)
    assert callable(ops.mask_stats) and callable(ops.nms) and hasattr(vdr.VitDescriptorModel, "generate_masks")
    assert hasattr(vdr, "MaskSet") and hasattr(vdr.Segmentation, "stats") and vdr.segment.MaskDecoder.LAUNCHES == 52
    # the partial slots: one of 8 int32 per band of at most 32 output rows; the suppression matrix: n x ceil(n / 64) words
    assert lib.vdr_mask_stats_workspace_bytes(192, 256, 256, 1024, 1024) == 192 * 32 * 32
    assert lib.vdr_mask_stats_workspace_bytes(1, 256, 256, 1, 1) == 32 and lib.vdr_mask_stats_workspace_bytes(1, 257, 1, 1, 1) == 0
    assert lib.vdr_nms_workspace_bytes(4096) == 4096 * 64 * 8 and lib.vdr_nms_workspace_bytes(65) == 65 * 2 * 8
    assert lib.vdr_nms_workspace_bytes(0) == 0 and lib.vdr_nms_workspace_bytes(4097) == 0


def test_both_entry_points_refuse_before_the_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 16384)()
    base = (C.addressof(raw) + 255) & ~255
    lg, ws, cn, bx = (base + 2048 * i for i in range(4))

    def ms(logits=lg, ps=64, ppg=1, gs=256, P=2, H=8, W=8, oh=32, ow=32, thr=0.0, off=1.0, work=ws, nbytes=2048, counts=cn, box=bx):
        return lib.vdr_op_mask_stats(logits, ps, ppg, gs, P, H, W, oh, ow, thr, off, work, nbytes, counts, box, None)
    for kw in (dict(logits=None), dict(work=None), dict(counts=None), dict(box=None), dict(logits=lg + 2), dict(work=ws + 8), dict(counts=cn + 4),
               dict(box=bx + 8), dict(H=0), dict(H=257), dict(W=0), dict(W=257), dict(oh=0), dict(oh=4097), dict(ow=0), dict(ow=4097), dict(P=0),
               dict(P=65536), dict(ps=63), dict(off=-1.0), dict(off=float("nan")), dict(ppg=0), dict(P=3, ppg=2), dict(P=4, ppg=2, gs=127)):
        assert ms(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_mask_stats: "), kw
    need = lib.vdr_mask_stats_workspace_bytes(2, 8, 8, 32, 32)
    assert need == 2 * 1 * 32 and ms(nbytes=need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_mask_stats: workspace too small")

    b, o, kp, kd = (base + 8192 + 512 * i for i in range(4))

    def nm(boxes=b, order=o, n=4, thr=0.5, work=ws, nbytes=2048, keep=kp, kept=kd, count=kd + 256):
        return lib.vdr_op_nms(boxes, order, n, thr, work, nbytes, keep, kept, count, None)
    for kw in (dict(boxes=None), dict(order=None), dict(work=None), dict(keep=None), dict(kept=None), dict(count=None), dict(n=0), dict(n=4097),
               dict(thr=float("nan")), dict(boxes=b + 4), dict(work=ws + 8), dict(order=o + 2), dict(kept=kd + 1), dict(count=kd + 258)):
        assert nm(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_nms: "), kw
    assert nm(nbytes=4 * 8 - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_nms: workspace too small")
    if not torch.cuda.is_available():
        assert ms() == -2 and ms(nbytes=need) == -2 and nm() == -2 and nm(nbytes=32) == -2   # VDR_ERR_NO_DEVICE, after every refusal above


# ---- the Python side ------------------------------------------------------------------------------------------------------------
class _Cfg:
    window, img, patch = 14, 128, 16


def _handle(decoder=True, points=True):
    h = types.SimpleNamespace(model_name="medsam", device="cpu", cfg=_Cfg(), has_mask_decoder=decoder)
    h.mask_decoder = types.SimpleNamespace(g=8, has_point_prompts=points, has_mask_prompt=True) if decoder else None
    return h


def test_generate_masks_refuses_before_any_device_work():
    import vdr
    gen = vdr.VitDescriptorModel.generate_masks
    x = torch.zeros((1, 3, 128, 128))
    with pytest.raises(ValueError, match="encoder-only checkpoint"):
        gen(_handle(decoder=False), x)
    with pytest.raises(ValueError, match="needs a SAM / MedSAM model"):
        gen(types.SimpleNamespace(model_name="vit", cfg=types.SimpleNamespace(window=0)), x)
    h = _handle()
    with pytest.raises(ValueError, match="one image a call"):
        gen(h, torch.zeros((2, 3, 128, 128)))
    with pytest.raises(ValueError, match="one image"):
        gen(h, torch.zeros((128, 128)))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="points_per_side"):
            gen(h, x, points_per_side=bad)
    for bad in (0, 65535, 1.0, False):
        with pytest.raises(ValueError, match="points_per_batch"):
            gen(h, x, points_per_batch=bad)
    for name in ("pred_iou_thresh", "stability_score_thresh", "stability_score_offset", "mask_threshold", "box_nms_thresh"):
        with pytest.raises(ValueError, match=name):
            gen(h, x, **{name: float("nan")})
        with pytest.raises(ValueError, match=name):
            gen(h, x, **{name: "high"})
    with pytest.raises(ValueError, match="stability_score_offset"):
        gen(h, x, stability_score_offset=-1.0)
    with pytest.raises(ValueError, match="weights absent"):
        gen(_handle(points=False), x)
    with pytest.raises(ValueError, match="size"):
        gen(h, x[0], size=(0, 128))                                                  # ([3, S, S] is taken; the size is not)
    from vdr import ops
    with pytest.raises(ValueError, match="mask_stats"):
        ops.mask_stats(torch.zeros((1, 8, 8)), (32, 32))                             # not on the device
    with pytest.raises(ValueError, match="nms"):
        ops.nms(torch.zeros((1, 4)), torch.zeros(1), 0.5)


def test_mask_set_methods_on_designed_logits():
    import vdr
    lg = torch.full((3, 4, 4), -1.0)
    lg[0, :, :] = 1.0                 # everything
    lg[1, :2, :2] = 1.0               # the top-left quarter
    lg[2, 2:, 2:] = 1.0               # the bottom-right quarter: the same area as mask 1
    ms = vdr.MaskSet(lg, torch.tensor([0.9, 0.8, 0.7]), torch.ones(3), torch.tensor([16, 4, 4], dtype=torch.int32),
                     torch.tensor([[0, 0, 3, 3], [0, 0, 1, 1], [2, 2, 3, 3]], dtype=torch.int32), torch.zeros((3, 2)), torch.arange(3), torch.zeros(3, dtype=torch.int64),
                     (16, 16), (4, 4), 0.0)
    assert len(ms) == 3 and ms.masks().dtype == torch.bool and tuple(ms.masks().shape) == (3, 4, 4) and tuple(ms.masks((8, 8)).shape) == (3, 8, 8)
    assert ms.boxes_xywh().tolist() == [[0, 0, 3, 3], [0, 0, 1, 1], [2, 2, 1, 1]]
    lm = ms.label_map()
    assert lm.dtype == torch.int32 and lm.tolist() == [[2, 2, 1, 1], [2, 2, 1, 1], [1, 1, 3, 3], [1, 1, 3, 3]]   # the small ones stay visible on the large one
    assert [r["counts"] for r in ms.rle()] == [[0, 16], [0, 2, 2, 2, 10], [10, 2, 2, 2]]
    empty = vdr.MaskSet(lg[:0], torch.zeros(0), torch.zeros(0), torch.zeros(0, dtype=torch.int32), torch.zeros((0, 4), dtype=torch.int32), torch.zeros((0, 2)),
                        torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), (16, 16), (4, 4), 0.0)
    assert len(empty) == 0 and tuple(empty.masks().shape) == (0, 4, 4) and int(empty.label_map().sum()) == 0 and empty.rle() == []


# ---- the mapping of the statistics kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_mask_stats_mapping_stages_in_bounds_and_owns_every_pixel_once(tmp_path, sanitize):
    """tests/mask_stats_map_cases.cpp, a host program with its own main, over the header the kernels include; the second build
    runs it under the address and undefined-behaviour sanitizers (host code, stand-alone)"""
    lines = host_program.run("mask_stats_map_cases", tmp_path, sanitize).splitlines()
    assert lines[-1] == "cases 48 fails 0"
    assert sum("unowned 0 twice 0" in ln and ln.endswith(")") and " bad 0 " in ln for ln in lines) == 48
    # the generator's shape (32 bands of 32 rows, 10 staged rows), a down-sampling that fills the stage, oh = 4096, sides of 1 and 256
    assert any(ln.startswith("P 3 H 256 W 256 oh 1024 ow 1024 layout 0: rows 32 bands 32 stage 10 ") for ln in lines)
    assert any(ln.startswith("P 3 H 256 W 256 oh 255 ow 257 layout 0: rows 28 bands 10 stage 29 ") for ln in lines)
    assert any(ln.startswith("P 6 H 256 W 8 oh 4096 ow 5 layout 1: rows 32 bands 128 stage 4 ") for ln in lines)
    assert any(ln.startswith("P 3 H 1 W 256 oh 7 ow 4096 layout 2: rows 32 bands 1 stage 1 ") for ln in lines)


# ---- the plane reduction the mask-plane kernels share ------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_plane_reduction_gives_brute_force_integers_in_every_order(tmp_path, sanitize):
    """tests/plane_reduce_cases.cpp, a host program with its own main, over csrc/plane_reduce.h: the identity is neutral, combine is
    commutative and associative on designed values, a slot round-trips, and a plane's pixels reduced forwards, reversed, as a tree
    and wave by wave give the brute-force counts and box; the second build runs it under the address and undefined-behaviour
    sanitizers (host code, stand-alone)"""
    lines = host_program.run("plane_reduce_cases", tmp_path, sanitize).splitlines()
    assert lines[-1] == "cases 24 fails 0"
    assert sum(ln.startswith("NS ") and ln.endswith(" designed 8 fails 0") for ln in lines) == 24
    assert all(f"NS {ns} W 517 H 300: " in "\n".join(lines) and f"NS {ns} W 1 H 1: " in "\n".join(lines) for ns in (1, 2, 3))
