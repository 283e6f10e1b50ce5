"""CPU: SAM's point and mask prompts without a device -- the restatements of tests/sam_prompt_ref.py against the
transformers.SamModel goldens (tests/golden/README_sam_prompts.md), the new C symbols (declared, bound, exported), the refusals
that need no handle (a handle cannot be made without a device: the handle-bound ones are in tests/test_sam_prompts_gpu.py), the
Python refusals, torch mask_box on designed masks, and the mapping of the fused keys kernel walked by a host program."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import host_program
import sam_decoder_ref as R
import sam_prompt_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {tag: PR.golden_prompts(golden_dir, tag) for tag in ("g8", "g10")}


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_restatements_reproduce_the_transformers_goldens(goldens, tag):
    """gates: 4 x the float64 mode's stored difference, 2 x the bf16 mode's; the spread condition of every set"""
    base, sets = goldens[tag]
    assert [s["name"] for s in sets] == ["point1", "points3", "box_points2", "box_refine"] + (["points10_mask", "box_point_pad"] if tag == "g10" else [])
    for s in sets:
        args = dict(boxes=s["boxes"], points=s["points"], labels=s["labels"], mask_input=s["mask_input"])
        got = R.diffs(*PR.decode(base["weights"], base["emb"], base["cfg"], mode="f64", **args), s["all4"], s["iou4"])
        print(f"{tag} {s['name']}: f64 restatement relL2 {got[0]:.3e} max|d| {got[1]:.3e} iou {got[2]:.3e} (stored {s['f64_diff']})")
        for v, stored in zip(got, s["f64_diff"]):
            assert v <= 4.0 * stored, s["name"]
        assert s["f64_diff"][0] < 1e-5
        got = R.diffs(*PR.decode(base["weights"], base["emb"], base["cfg"], mode="bf16", **args), s["all4"], s["iou4"])
        for v, stored in zip(got, s["bf16_diff"]):
            assert v <= 2.0 * stored, s["name"]
        assert float((s["all4"].abs() < 2.0 * s["bf16_diff"][1]).double().mean()) <= 0.10, s["name"]
    by = {s["name"]: s for s in sets}
    if tag == "g10":
        assert tuple(by["points10_mask"]["points"].shape) == (1, 3, 10, 2) and tuple(by["points10_mask"]["mask_input"].shape) == (1, 40, 40)
        assert -10 in by["box_point_pad"]["labels"].tolist()[0][1]
    assert torch.equal(by["box_refine"]["mask_input"], base["pred_masks_single"][:, 0, 0])   # the box case's own logits, fed back


def test_restatement_with_boxes_only_is_the_box_restatement(goldens):
    base, _ = goldens["g10"]
    a = PR.decode(base["weights"], base["emb"], base["cfg"], boxes=base["boxes"], mode="bf16")
    b = R.decode(base["weights"], base["emb"], base["boxes"], base["cfg"], "bf16")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_point_rows_follow_the_label_table(goldens):
    base, _ = goldens["g8"]
    w = base["weights"]
    pts = torch.tensor([[[[10.0, 20.0], [10.0, 20.0], [10.0, 20.0], [10.0, 20.0], [10.0, 20.0]]]])
    rows = PR.sparse_tokens(w, 128, None, pts, torch.tensor([[[1, 0, -1, -10, 5]]]))[0]
    pe = R.fourier_pe((pts[0, 0, :1].double() + 0.5) / 128.0, w["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"])[0]
    nap = w["prompt_encoder.not_a_point_embed.weight"][0].double()
    assert rows.shape == (6, 256)                                                             # 5 points + the padding row
    assert torch.equal(rows[0], pe + w["prompt_encoder.point_embeddings.1.weight"][0].double())
    assert torch.equal(rows[1], pe + w["prompt_encoder.point_embeddings.0.weight"][0].double())
    assert torch.equal(rows[2], nap) and torch.equal(rows[3], torch.zeros(256, dtype=torch.float64))
    assert torch.equal(rows[4], pe) and torch.equal(rows[5], nap)                             # any other label: the pe alone
    both = PR.sparse_tokens(w, 128, torch.tensor([[[1.0, 2.0, 30.0, 40.0]]]), pts, torch.tensor([[[1, 0, -1, -10, 5]]]))[0]
    assert both.shape == (7, 256) and torch.equal(both[:5], rows[:5]) and torch.equal(both[5:], R.box_tokens(torch.tensor([[[1.0, 2.0, 30.0, 40.0]]]), 128, w)[0])


def test_mask_embed_restatement_is_the_convolution_chain(goldens):
    base, _ = goldens["g8"]
    w = base["weights"]
    g = torch.Generator().manual_seed(5)
    emb, mask = torch.randn((2, 256, 3, 3), generator=g), 3.0 * torch.randn((2, 12, 12), generator=g)
    exact, bound = PR.mask_embed_ref(emb, mask, w, 1e-6)
    want = (emb.double() + PR.mask_dense(w, mask, 1e-6)).permute(0, 2, 3, 1).reshape(-1, 256)
    assert float((exact - want).abs().max()) < 1e-12 and bool((bound > 0).all()) and float(bound.max()) < 1e-2
    assert tuple(PR.pack_mask_weights(w).shape) == (4684,)
    shared, _ = PR.mask_embed_ref(emb[:1], mask[:1], w, 1e-6, nb=3)                            # one mask for the image's 3 problems
    assert torch.equal(shared[:9], shared[9:18]) and torch.equal(shared[:9], exact[:9])


def test_torch_mask_box_on_designed_masks():
    lg = torch.full((4, 8, 8), -1.0)
    lg[1, 2, 5] = 1.0                                  # a single pixel
    lg[2] = 1.0                                        # full
    lg[3, 0, 0] = lg[3, 7, 7] = 0.5                    # two corners
    prev = torch.tensor([[1.0, 2.0, 3.0, 4.0]] * 4)
    box, area = PR.mask_box_ref(lg, prev, 128, margin=8.0)
    assert area.tolist() == [0, 1, 64, 2] and area.dtype == torch.int32
    assert box[0].tolist() == [1.0, 2.0, 3.0, 4.0]                                            # empty: prev
    assert box[1].tolist() == [5 * 16.0 - 8, 2 * 16.0 - 8, 6 * 16.0 + 8, 3 * 16.0 + 8]
    assert box[2].tolist() == [0.0, 0.0, 128.0, 128.0] and box[3].tolist() == [0.0, 0.0, 128.0, 128.0]   # clamped at the border
    assert PR.mask_box_ref(lg, prev, 128, threshold=0.75)[1].tolist() == [0, 1, 64, 0]


# ---- the C side ----------------------------------------------------------------------------------------------------------------
NEW = ("vdr_mask_decoder_num_prompt_weights", "vdr_mask_decoder_prompt_support", "vdr_mask_decoder_workspace_bytes_prompts",
       "vdr_mask_decode_prompts", "vdr_op_mask_embed", "vdr_op_mask_box")


def test_new_symbols_are_declared_bound_and_exported():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "vdr_mask_decoder_prompt_weight_name" in _lib.SYMBOLS and hasattr(lib, "vdr_mask_decoder_prompt_weight_name")
    assert lib.vdr_abi_version() == 8 and "#define VDR_ABI_VERSION 8" in src                   # additive: the version stays
    assert C.sizeof(_lib.vdr_mask_prompts) == 48 and _lib.MASK_EMBED_WEIGHTS == 4 * 4 + 3 * 4 + 16 * 16 + 3 * 16 + 256 * 16 + 256
    assert re.search(r"#define VDR_MASK_EMBED_WEIGHTS 4684\b", src)
    for name in ("mask_embed", "mask_box"):
        assert callable(getattr(ops, name))
    for name in ("propagate_masks", "segment", "decode_masks"):
        assert hasattr(vdr.VitDescriptorModel, name)
    assert callable(vdr.pipeline.propagate_segmentation) and vdr.segment.MaskDecoder.LAUNCHES == 52 and vdr.segment.MAX_TOKENS == 16
    assert hasattr(vdr, "VolumeSegmentation") and hasattr(vdr.Segmentation, "best") and hasattr(vdr.Segmentation, "as_mask_input")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^NOCONTRACT :=.*\bmask_prompt\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\bmask_prompt\.hip\b", mk, re.M)
    assert re.search(r"^ASM :=.*\bmask_prompt\b", mk, re.M)


def test_prompt_refusals_come_before_the_handle_and_the_device():
    """no prompt at all and T = 17 are refused from the prompts struct alone, first of all: without a device there is no handle
    to give (vdr_mask_decoder_create is VDR_ERR_NO_DEVICE), and the refusal must still be the prompts'"""
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 4096)()
    base = (C.addressof(raw) + 255) & ~255
    n = C.c_size_t()

    def dec(pr, h=None):
        return lib.vdr_mask_decode_prompts(h, base, 0, C.byref(pr) if pr is not None else None, 1, 1, base + 256, 256, base + 512, base + 768, None)
    assert dec(None) == -1
    assert dec(_lib.vdr_mask_prompts()) == -1 and b"at least one of boxes and points" in lib.vdr_last_error(None)
    assert dec(_lib.vdr_mask_prompts(mask_input=base)) == -1 and b"at least one of boxes and points" in lib.vdr_last_error(None)
    assert dec(_lib.vdr_mask_prompts(points=base)) == -1 and b"labels" in lib.vdr_last_error(None)
    assert dec(_lib.vdr_mask_prompts(points=base, labels=base, points_per_problem=0)) == -1
    assert dec(_lib.vdr_mask_prompts(boxes=base, mask_per_image=2)) == -1
    for pr in (_lib.vdr_mask_prompts(boxes=base, points=base, labels=base, points_per_problem=10),          # T = 17 with a box
               _lib.vdr_mask_prompts(points=base, labels=base, points_per_problem=11)):                     # T = 17 without
        assert dec(pr) == -7 and b"at most 16 tokens" in lib.vdr_last_error(None) and b"got 17" in lib.vdr_last_error(None)
    assert lib.vdr_last_error(None).startswith(b"vdr_mask_decode_prompts: ")
    # well-formed prompts get as far as the handle check
    assert dec(_lib.vdr_mask_prompts(boxes=base, points=base, labels=base, points_per_problem=9)) == -1 and b"null argument" in lib.vdr_last_error(None)
    assert lib.vdr_mask_decoder_workspace_bytes_prompts(None, 1, 17, C.byref(n)) == -7
    assert lib.vdr_mask_decoder_workspace_bytes_prompts(None, 1, 5, C.byref(n)) == -1
    assert lib.vdr_mask_decoder_workspace_bytes_prompts(None, 1, 7, C.byref(n)) == -1 and b"null handle" in lib.vdr_last_error(None)
    assert lib.vdr_mask_decoder_num_prompt_weights(None) == 0 and lib.vdr_mask_decoder_prompt_weight_name(None, 0) is None
    assert lib.vdr_mask_decoder_prompt_support(None) == 0


def test_op_refusals_come_before_the_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    e, m, w, k = (base + 1024 * i for i in range(4))

    def me(emb=e, cl=0, mask=m, mpi=0, wt=w, keys=k, P=2, nb=1, g=3, eps=1e-6):
        return lib.vdr_op_mask_embed(emb, cl, mask, mpi, wt, keys, P, nb, g, eps, None)
    for kw in (dict(g=0), dict(g=65)):
        assert me(**kw) == -7, kw
    for kw in (dict(emb=None), dict(mask=None), dict(wt=None), dict(keys=None), dict(cl=2), dict(mpi=-1), dict(P=0), dict(P=70000), dict(nb=0),
               dict(P=3, nb=2), dict(eps=0.0), dict(emb=e + 4), dict(mask=m + 8), dict(keys=k + 2)):
        assert me(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_mask_embed: ")

    def mb(lg=e, stride=64, prev=m, boxes=w, area=k, P=2, H=8, W=8, img=128, margin=8.0, thr=0.0):
        return lib.vdr_op_mask_box(lg, stride, prev, boxes, area, P, H, W, img, margin, thr, None)
    for kw in (dict(img=(1 << 24) + 1), dict(H=1 << 16, W=1 << 16, stride=1 << 40)):
        assert mb(**kw) == -7, kw
    for kw in (dict(lg=None), dict(prev=None), dict(boxes=None), dict(area=None), dict(P=0), dict(P=70000), dict(H=0), dict(W=-1), dict(img=0),
               dict(stride=63), dict(margin=-1.0), dict(margin=float("nan")), dict(thr=float("nan")), dict(lg=e + 2), dict(prev=m + 4), dict(boxes=w + 8)):
        assert mb(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_mask_box: ")
    if not torch.cuda.is_available():
        assert me() == -2 and mb() == -2 and mb(stride=256) == -2              # VDR_ERR_NO_DEVICE, after every refusal above


# ---- the Python side ------------------------------------------------------------------------------------------------------------
class _Cfg:
    window, img, patch = 14, 128, 16


def _handle(points=True, mask=True):
    h = types.SimpleNamespace(model_name="medsam", device="cpu", cfg=_Cfg(), has_mask_decoder=True)
    h.mask_decoder = types.SimpleNamespace(g=8, has_point_prompts=points, has_mask_prompt=mask)
    return h


def test_python_calls_refuse_before_any_device_work():
    import vdr
    M = vdr.VitDescriptorModel
    x, emb = torch.zeros((1, 3, 128, 128)), torch.zeros((1, 256, 8, 8))
    boxes, pts, lbl = torch.zeros((1, 2, 4)), torch.zeros((1, 2, 3, 2)), torch.ones((1, 2, 3), dtype=torch.int64)
    h = _handle()
    for call in (lambda **kw: M.segment(h, x, **kw), lambda **kw: M.decode_masks(h, emb, **kw)):
        with pytest.raises(ValueError, match="no prompt"):
            call()
        with pytest.raises(ValueError, match="no prompt"):
            call(mask_input=torch.zeros((1, 32, 32)))
        with pytest.raises(ValueError, match="go together"):
            call(points=pts)
        with pytest.raises(ValueError, match="nb mismatch"):
            call(boxes=boxes, points=torch.zeros((1, 3, 1, 2)), point_labels=torch.ones((1, 3, 1), dtype=torch.int64))
        with pytest.raises(ValueError, match="17 tokens"):
            call(boxes=boxes, points=torch.zeros((1, 2, 10, 2)), point_labels=torch.ones((1, 2, 10), dtype=torch.int64))
        with pytest.raises(ValueError, match="17 tokens"):
            call(points=torch.zeros((1, 2, 11, 2)), point_labels=torch.ones((1, 2, 11), dtype=torch.int64))
        for bad in (torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3, 3)), torch.zeros((1, 2, 0, 2)), torch.zeros((2, 2, 3, 2))):
            with pytest.raises(ValueError, match="points|point sets|point_labels"):
                call(points=bad, point_labels=lbl)
        with pytest.raises(ValueError, match="point_labels must be"):
            call(points=pts, point_labels=torch.ones((1, 2, 2), dtype=torch.int64))
        with pytest.raises(ValueError, match="integers"):
            call(points=pts, point_labels=torch.ones((1, 2, 3)))
        with pytest.raises(ValueError, match="1 .foreground."):
            call(points=pts, point_labels=torch.full((1, 2, 3), 2))
        for bad in (torch.zeros((1, 2, 16, 16)), torch.zeros((1, 3, 32, 32)), torch.zeros((2, 32, 32)), torch.zeros((32, 32)),
                    torch.zeros((1, 2, 32, 32), dtype=torch.int32)):
            with pytest.raises(ValueError, match="wrong mask shape"):
                call(boxes=boxes, mask_input=bad)
    bare = _handle(points=False, mask=False)
    with pytest.raises(ValueError, match="weights absent"):
        M.decode_masks(bare, emb, points=pts, point_labels=lbl)
    with pytest.raises(ValueError, match="weights absent"):
        M.decode_masks(bare, emb, boxes, mask_input=torch.zeros((1, 2, 32, 32)))
    with pytest.raises(ValueError, match="weights absent"):
        M.propagate_masks(bare, x, [1, 2, 30, 40], 0)                                        # use_mask_prompt=True by default
    for kw, match in ((dict(index=1), "index"), (dict(index=-1), "index"), (dict(index=0, direction="left"), "direction"),
                      (dict(index=0, margin=-1), "margin"), (dict(index=0, max_batch=0), "max_batch")):
        with pytest.raises(ValueError, match=match):
            M.propagate_masks(h, x, [1, 2, 30, 40], **kw)
    with pytest.raises(ValueError, match="box must be"):
        M.propagate_masks(h, x, [1, 2, 30], 0)
    with pytest.raises(ValueError, match="index"):
        vdr.pipeline.propagate_segmentation(h, np.zeros((20, 30, 2), np.float32), [1, 2, 3, 4], 2)
    with pytest.raises(ValueError, match="img_3d"):
        vdr.pipeline.propagate_segmentation(h, np.zeros((20, 30), np.float32), [1, 2, 3, 4], 0)
    with pytest.raises(ValueError, match="go together"):
        vdr.segment_slice(h, np.zeros((20, 30), np.float32), points=[[1, 2]])
    with pytest.raises(ValueError, match=r"\[np, 2\]"):
        vdr.segment_slice(h, np.zeros((20, 30), np.float32), points=[1, 2], point_labels=[1])
    with pytest.raises(ValueError, match="no prompt"):
        vdr.segment_slice(h, np.zeros((20, 30), np.float32))
    from vdr import ops
    with pytest.raises(ValueError, match="mask_embed"):
        ops.mask_embed(torch.zeros((1, 256, 2, 2)), torch.zeros((1, 8, 8)), torch.zeros(4684))
    with pytest.raises(ValueError, match="mask_box"):
        ops.mask_box(torch.zeros((1, 8, 8)), torch.zeros((1, 4)), 128)


def test_best_and_as_mask_input_select_per_problem():
    import vdr
    lg = torch.arange(2 * 1 * 3 * 4 * 4, dtype=torch.float32).reshape(2, 1, 3, 4, 4)
    iou = torch.tensor([[[0.125, 0.875, 0.5]], [[0.75, 0.75, 0.25]]])
    seg = vdr.Segmentation(lg, iou, (16, 16))
    best = seg.best()
    assert tuple(best.low_res_logits.shape) == (2, 1, 1, 4, 4) and best.iou.tolist() == [[[0.875]], [[0.75]]]
    assert torch.equal(best.low_res_logits[0, 0, 0], lg[0, 0, 1]) and torch.equal(best.low_res_logits[1, 0, 0], lg[1, 0, 0])   # a tie: the lowest index
    assert torch.equal(seg.as_mask_input(), best.low_res_logits[:, :, 0]) and torch.equal(seg.as_mask_input(2), lg[:, :, 2])
    for bad in (3, -1, "first", True):
        with pytest.raises(ValueError, match="select"):
            seg.as_mask_input(bad)
    vol = vdr.VolumeSegmentation(lg[:, 0, 0], iou[:, 0, 0], torch.zeros((2, 4)), torch.zeros(2, dtype=torch.int32), (16, 16))
    assert tuple(vol.masks().shape) == (2, 16, 16) and vol.masks().dtype == torch.bool and tuple(vol.logits((5, 7)).shape) == (2, 5, 7)


# ---- the mapping of the fused keys kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_mask_embed_mapping_reads_in_bounds_and_writes_every_key_once(tmp_path, sanitize):
    """tests/mask_embed_map_cases.cpp, a host program with its own main, over the header the kernel includes; the second build
    runs it under the address and undefined-behaviour sanitizers (host code, stand-alone)"""
    lines = host_program.run("mask_embed_map_cases", tmp_path, sanitize).splitlines()
    assert lines[-1] == "cases 64 fails 0"
    assert sum("unwritten 0 twice 0" in ln for ln in lines) == 64
    # ragged last tile (g 3, P 3: 27 rows), tiles that span two problems (g 10: 100 rows a problem), the largest grid
    assert any(ln.startswith("g 3 P 3 nb 1 channels_last 0 mask_per_image 0: tiles 1 rows 27") for ln in lines)
    assert any(ln.startswith("g 10 P 5 nb 1 channels_last 1 mask_per_image 1: tiles 16 rows 500") for ln in lines)
    assert any(ln.startswith("g 64 P 3 nb 3 channels_last 0 mask_per_image 1: tiles 384 rows 12288") for ln in lines)
