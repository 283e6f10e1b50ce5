"""GPU: SAM's point and mask prompts -- the fused keys kernel (vdr_op_mask_embed) inside the entry-wise fp32 bound of
tests/sam_prompt_ref.py and its bitwise properties, vdr_op_mask_box bit for bit against its torch statement, the decode with
every prompt kind against the transformers.SamModel goldens (gates stored in the golden files: 2 x the CPU-measured difference
of the restatement's bf16 mode; tests/golden/README_sam_prompts.md), the token rows, the handle's optional weights and memory
contract, and the volume sweep model.propagate_masks against a hand loop.  Nothing is derived from device output."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import handle_configs as hc
import memguard as mg
import sam_decoder_ref as R
import sam_prompt_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- mask_embed ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pw():
    w = PR.draw_prompt_weights(7)
    return w, PR.pack_mask_weights(w).to(DEV)


@pytest.mark.parametrize("g,P", [(1, 3), (3, 3), (10, 3), (64, 1)])
def test_mask_embed_stays_inside_its_bound(pw, g, P):
    """g = 1 and 3: 3 and 27 rows, below one 32-row tile; g = 10: 300 rows, tiles that span two problems and a ragged last one;
    g = 64: 4096 rows.  The output lies between canary rows."""
    from vdr import ops
    w, packed = pw
    emb, mask = _randn((P, 256, g, g), 1), _randn((P, 4 * g, 4 * g), 2, 3.0)
    whole, body = mg.guarded_rows(P * g * g, 256, torch.bfloat16)
    out = ops.mask_embed(emb.to(DEV), mask.to(DEV), packed, eps=1e-6, out=body)
    torch.cuda.synchronize()
    assert mg.rows_intact(whole, 8) and mg.canary_left(body) == 0
    exact, bound = PR.mask_embed_ref(emb, mask, w, 1e-6)
    got = out.double().cpu()
    off = (got - R.bf16(exact)).abs() > 0
    # how far outside [bf16(exact - bound), bf16(exact + bound)] in units of the bound (<= 0: inside), and the plain error
    lo, hi = R.bf16(exact - bound), R.bf16(exact + bound)
    worst = float((torch.maximum(lo - got, got - hi) / bound).max())
    print(f"mask_embed g {g} P {P}: {int(off.sum())} of {off.numel()} outputs off bf16(exact); max bound {float(bound.max()):.3e}; "
          f"worst (distance outside the bound's bf16 interval) / bound {worst:.3f} (<= 0: inside)")
    assert R.within_bf16_of(out, exact, bound)


def test_mask_embed_with_a_zero_last_convolution_is_emb_plus_bias_exactly(pw):
    from vdr import ops
    w = dict(pw[0])
    w[PR.MD + "6.weight"] = torch.zeros_like(w[PR.MD + "6.weight"])
    g, P = 10, 3
    emb, mask = _randn((P, 256, g, g), 3), _randn((P, 4 * g, 4 * g), 4, 3.0)
    out = ops.mask_embed(emb.to(DEV), mask.to(DEV), PR.pack_mask_weights(w).to(DEV))
    want = (emb.permute(0, 2, 3, 1).reshape(-1, 256) + w[PR.MD + "6.bias"]).to(torch.bfloat16)   # one fp32 addition, one rounding
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_mask_embed_bits_depend_neither_on_the_call_nor_on_the_layout(pw):
    from vdr import ops
    _, packed = pw
    g, B, nb = 10, 2, 3
    n = g * g
    emb, mask = _randn((B, 256, g, g), 5).to(DEV), _randn((B * nb, 4 * g, 4 * g), 6, 3.0).to(DEV)
    full = ops.mask_embed(emb, mask, packed, problems_per_image=nb)
    assert torch.equal(full, ops.mask_embed(emb, mask, packed, problems_per_image=nb))
    for p in range(B * nb):                                                     # a problem alone
        one = ops.mask_embed(emb[p // nb:p // nb + 1], mask[p:p + 1], packed)
        assert torch.equal(one, full[p * n:(p + 1) * n]), p
    cl = emb.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)               # the encoder's own layout, read in place
    assert not cl.is_contiguous() and torch.equal(ops.mask_embed(cl, mask, packed, problems_per_image=nb), full)
    shared = ops.mask_embed(emb, mask[::nb].contiguous(), packed, problems_per_image=nb)   # one mask per image ...
    again = ops.mask_embed(emb, mask[::nb].repeat_interleave(nb, dim=0), packed, problems_per_image=nb)   # ... is the repeated mask
    assert torch.equal(shared, again)
    assert torch.equal(ops.mask_embed(cl, mask[::nb].contiguous(), packed, problems_per_image=nb), again)


# ---- mask_box ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 5, 32, 40, 256])   # (5: a width that is no multiple of 4 takes the scalar loads)
def test_mask_box_equals_its_torch_statement_bit_for_bit(S):
    from vdr import ops
    img = 1024 if S == 256 else 160
    lg = torch.full((8, 4, S, S), -1.0)
    lg[1, 0, 0, 0] = lg[2, 0, 0, S - 1] = lg[3, 0, S - 1, 0] = lg[4, 0, S - 1, S - 1] = 2.0     # a single pixel at each corner
    lg[5, 0] = 1.0                                                                               # full
    lg[6, 0] = _randn((S, S), 11)                                                                # random
    lg[7, 0, S // 2:, 1:S // 2 + 1] = 0.25                                                       # a block off the left border
    lg[:, 1:] = _randn((8, 3, S, S), 12)                                                         # the other tokens: never read
    lg = lg.to(DEV)
    prev = _randn((8, 4), 13, 50.0).abs().to(DEV)
    for margin, thr in ((0.0, 0.0), (8.0, 0.0), (3.5, 0.5), (2000.0, 0.0)):                      # the last: everything clamps
        box, area = ops.mask_box(lg[:, 0], prev, img, margin=margin, threshold=thr)              # token 0 read in place (strided planes)
        want_box, want_area = PR.mask_box_ref(lg[:, 0], prev, img, margin, thr)
        torch.cuda.synchronize()
        assert box.dtype == torch.float32 and area.dtype == torch.int32
        assert torch.equal(box.view(torch.int32), want_box.view(torch.int32)) and torch.equal(area, want_area), (margin, thr)
        dense_box, dense_area = ops.mask_box(lg[:, 0].contiguous(), prev, img, margin=margin, threshold=thr)
        assert torch.equal(dense_box, box) and torch.equal(dense_area, area)
    box, area = ops.mask_box(lg[:, 0], prev, img, margin=8.0)
    assert torch.equal(box[0], prev[0]) and int(area[0]) == 0 and int(area[5]) == S * S         # empty: prev's box
    assert box[1].tolist() == [0.0, 0.0, img / S + 8.0, img / S + 8.0] and box[5].tolist() == [0.0, 0.0, float(img), float(img)]


@pytest.mark.parametrize("H,W,last,pair", [(256, 256, (3, 255), ((0, 1), (3, 200))),   # 4 pixels a load: thread 255 owns pixels 1020 .. 1023
                                           (40, 7, (36, 3), ((0, 2), (28, 4)))])       # W = 7, one pixel a load: thread 255 owns pixel 255
def test_mask_box_reduces_the_last_thread_and_the_outer_waves(H, W, last, pair):
    """the workgroup's reduction at its edges: the only pixel above threshold belongs to thread 255 (the last lane of the last
    wave); a pair that waves 0 and 3 own; an empty plane, which returns prev.  (y, x) pixels; the other threads stay at the
    identity"""
    from vdr import ops
    lg = torch.full((3, H, W), -1.0)
    lg[0, last[0], last[1]] = 2.0
    for y, x in pair:
        lg[1, y, x] = 2.0
    lg = lg.to(DEV)
    prev = _randn((3, 4), 17, 50.0).abs().to(DEV)
    for margin in (0.0, 3.5):
        box, area = ops.mask_box(lg, prev, 1024, margin=margin)
        want_box, want_area = PR.mask_box_ref(lg, prev, 1024, margin, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(box.view(torch.int32), want_box.view(torch.int32)) and torch.equal(area, want_area), margin
        assert area.tolist() == [1, 2, 0] and torch.equal(box[2], prev[2])
    box, _ = ops.mask_box(lg, prev, 1024)
    sx, sy = 1024 / W, 1024 / H                                                                   # (exact in fp32 for 256; the reference holds W = 7)
    if W == 256:
        assert box[0].tolist() == [last[1] * sx, last[0] * sy, (last[1] + 1) * sx, (last[0] + 1) * sy]
        assert box[1].tolist() == [1 * sx, 0.0, 201 * sx, 4 * sy]


# ---- the decode ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {tag: PR.golden_prompts(golden_dir, tag) for tag in ("g8", "g10")}


@contextlib.contextmanager
def _model(c, name, drop=()):
    import vdr
    from oracle import sam_oracle as so
    cfg = so.SamCfg(c["cfg"].img, 16, 3, 64, 1, 2, 128, 4, (1,), 256, 1e-6)
    vdr.ARCHS[name] = hc.sam_config(cfg)
    try:
        w = dict(so.make_weights(cfg, seed=c["wseed"], scale=0.05))
        w.update({k: v for k, v in c["weights"].items() if not k.startswith(drop)})
        yield vdr.load_model(name, weights=w, decoder_eps=c["eps"])
    finally:
        del vdr.ARCHS[name]


@pytest.fixture(scope="module")
def models(goldens):
    with contextlib.ExitStack() as st:
        yield {tag: st.enter_context(_model(base, "sam_prompts_" + tag)) for tag, (base, _) in goldens.items()}


@pytest.fixture(scope="module")
def box_only(goldens):
    """the g8 checkpoint without mask_downscaling.* and without not_a_point_embed: boxes alone"""
    with _model(goldens["g8"][0], "sam_prompts_box_only", drop=(PR.MD, "prompt_encoder.not_a_point_embed")) as m:
        yield m


def _all4(m, emb, **kw):
    multi, single = m.decode_masks(emb, multimask=True, **kw), m.decode_masks(emb, **kw)
    return torch.cat([single.low_res_logits, multi.low_res_logits], dim=2), torch.cat([single.iou, multi.iou], dim=2)


@pytest.mark.parametrize("tag", ["g8", "g10"])
def test_every_prompt_set_passes_its_stored_gate(goldens, models, tag):
    (base, sets), m = goldens[tag], models[tag]
    assert m.mask_decoder.has_point_prompts and m.mask_decoder.has_mask_prompt and m.mask_decoder.LAUNCHES == 52
    emb = base["emb"].to(DEV)
    for s in sets:
        lg, iou = _all4(m, emb, boxes=s["boxes"], points=s["points"], point_labels=s["labels"], mask_input=s["mask_input"])
        torch.cuda.synchronize()
        rel, mx, di = R.diffs(lg, iou, s["all4"], s["iou4"])
        g_rel, g_abs, g_iou = (2.0 * v for v in s["bf16_diff"])
        print(f"decode {tag} {s['name']}: relL2 {rel:.3e} (gate {g_rel:.3e})  max|d| {mx:.3e} (gate {g_abs:.3e})  iou head {di:.3e} (gate {g_iou:.3e})")
        assert rel <= g_rel and mx <= g_abs and di <= g_iou, s["name"]
        clear = s["all4"].abs() > g_abs                                         # the masks: IoU 1 over the pixels clear of zero
        assert float((~clear).double().mean()) <= 0.10
        assert torch.equal((lg.cpu() > 0)[clear], (s["all4"] > 0)[clear]), s["name"]


@pytest.mark.parametrize("T", [8, 9, 16])
def test_decode_follows_the_bf16_restatement_at_other_token_counts(goldens, models, T):
    """T = 8: a box and one point; 9: three points and the padding row; 16: a box and nine points (the layout has no T = 6: the
    smallest decode is 5 + 2 box corners or 5 + one point + the padding row).  Gate: with b = |bf16 mode - float64 mode| of the
    restatement on these inputs (CPU), the device is allowed 2 b from the definition (the golden gates' rule), so 3 b from the
    bf16 mode."""
    (base, _), m = goldens["g8"], models["g8"]
    B, img = 2, base["cfg"].img
    rs = np.random.RandomState(40 + T)
    npts = {8: 1, 9: 3, 16: 9}[T]
    points = torch.from_numpy(rs.uniform(0.0, img, size=(B, 1, npts, 2)).astype(np.float32))
    labels = torch.from_numpy(rs.randint(0, 2, size=(B, 1, npts)).astype(np.int32))
    boxes = None if T == 9 else base["boxes"]
    lg, iou = m.mask_decoder.decode(base["emb"].to(DEV), boxes, points, labels)
    args = dict(boxes=boxes, points=points, labels=labels)
    f = PR.decode(base["weights"], base["emb"], base["cfg"], mode="f64", **args)
    b = PR.decode(base["weights"], base["emb"], base["cfg"], mode="bf16", **args)
    gate = R.diffs(b[0], b[1], f[0], f[1])
    got = R.diffs(lg, iou, b[0], b[1])
    print(f"T {T}: device vs bf16 mode relL2 {got[0]:.3e} max|d| {got[1]:.3e} iou {got[2]:.3e}; bf16 mode vs float64 {gate}")
    for v, gt in zip(got, gate):
        assert v <= 3.0 * gt


def _raw_decode(d, emb, pr, B, nb, T, ws=None):
    need = d.workspace_bytes(B * nb, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if ws is None else ws
    lg = torch.empty((B, nb, 4, 4 * d.g, 4 * d.g), device=DEV)
    iou = torch.empty((B, nb, 4), device=DEV)
    rc = d.lib.vdr_mask_decode_prompts(d.h, emb.data_ptr(), 0, C.byref(pr), B, nb, ws.data_ptr(), ws.numel(), lg.data_ptr(), iou.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    return rc, lg, iou, ws


def test_boxes_only_through_the_new_entry_point_is_vdr_mask_decode_bit_for_bit(goldens, models):
    from vdr import _lib
    for tag in ("g8", "g10"):
        (base, _), m = goldens[tag], models[tag]
        d = m.mask_decoder
        emb, boxes = base["emb"].to(DEV).contiguous(), base["boxes"].to(DEV).float().contiguous()
        B, nb = boxes.shape[:2]
        rc, lg, iou, _ = _raw_decode(d, emb, _lib.vdr_mask_prompts(boxes=boxes.data_ptr()), B, nb, 7)
        want_lg, want_iou = d.decode(emb, base["boxes"])
        assert rc == 0 and torch.equal(lg, want_lg) and torch.equal(iou, want_iou)
        assert d.workspace_bytes(B * nb, 7) == d.workspace_bytes(B * nb)


def test_token_rows_follow_the_label_table_and_a_not_a_point_row_changes_no_other(goldens, models):
    """the workspace begins with the tokens as set up (include/vdr.h): rows 5.. against the restatement, rounded once"""
    from vdr import _lib
    (base, _), m = goldens["g8"], models["g8"]
    d, w = m.mask_decoder, base["weights"]
    emb = base["emb"].to(DEV).contiguous()
    B, nb = 2, 1
    pts = torch.tensor([[[[10.0, 20.0], [100.5, 3.25], [64.0, 64.0], [0.0, 127.0], [77.0, 5.0]]], [[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0]]]])
    lbl = torch.tensor([[[1, 0, -1, -10, 5]], [[0, 0, 1, -1, 1]]], dtype=torch.int32)

    def tokens(points, labels, boxes=None):
        p, lb = points.to(DEV).contiguous(), labels.to(DEV).contiguous()
        bx = None if boxes is None else boxes.to(DEV).float().contiguous()
        T = 5 + points.shape[2] + (2 if boxes is not None else 1)
        pr = _lib.vdr_mask_prompts(boxes=None if bx is None else bx.data_ptr(), points=p.data_ptr(), labels=lb.data_ptr(), points_per_problem=points.shape[2])
        rc, lg, iou, ws = _raw_decode(d, emb, pr, B, nb, T)
        torch.cuda.synchronize()
        assert rc == 0
        return ws[:B * nb * T * 256 * 2].view(torch.bfloat16).view(B * nb, T, 256).cpu(), lg, iou
    tok, _, _ = tokens(pts, lbl)
    fixed = torch.cat([w["mask_decoder.iou_token.weight"], w["mask_decoder.mask_tokens.weight"]], 0).to(torch.bfloat16)
    want = PR.sparse_tokens(w, base["cfg"].img, None, pts, lbl).float().to(torch.bfloat16)       # float(double), then one rounding to bf16
    assert tok.shape == (2, 11, 256) and torch.equal(tok[:, :5], fixed[None].expand(2, -1, -1))
    assert torch.equal(tok[:, 5:].view(torch.int16), want.view(torch.int16))
    nap = w["prompt_encoder.not_a_point_embed.weight"][0].to(torch.bfloat16)
    assert torch.equal(tok[0, 7], nap) and torch.equal(tok[0, 10], nap) and not bool(tok[0, 8].any())   # -1, the padding row, -10
    # with a box: no padding row, the corners last
    tokb, _, _ = tokens(pts, lbl, base["boxes"])
    wantb = PR.sparse_tokens(w, base["cfg"].img, base["boxes"], pts, lbl).float().to(torch.bfloat16)
    assert tokb.shape == (2, 12, 256) and torch.equal(tokb[:, 5:].view(torch.int16), wantb.view(torch.int16))
    # one more point labelled -1: every other row keeps its bits, the new row is not_a_point_embed
    more_p = torch.cat([pts[:, :, :2], torch.tensor([[[[50.0, 60.0]]], [[[70.0, 80.0]]]])], dim=2)
    more_l = torch.cat([lbl[:, :, :2], torch.full((2, 1, 1), -1, dtype=torch.int32)], dim=2)
    t2, _, _ = tokens(pts[:, :, :2].contiguous(), lbl[:, :, :2].contiguous())
    t3, _, _ = tokens(more_p, more_l)
    assert t2.shape[1] == 8 and t3.shape[1] == 9 and torch.equal(t3[:, :7], t2[:, :7]) and torch.equal(t3[:, 8], t2[:, 7])
    assert torch.equal(t3[:, 7], nap[None].expand(2, -1))


def test_problem_bits_do_not_depend_on_the_call_at_16_tokens(goldens, models):
    (base, sets), m = goldens["g10"], models["g10"]
    s = {x["name"]: x for x in sets}["points10_mask"]
    emb = base["emb"].to(DEV)
    lg, iou = m.mask_decoder.decode(emb, None, s["points"], s["labels"], s["mask_input"])
    again = m.mask_decoder.decode(emb, None, s["points"], s["labels"], s["mask_input"])
    assert torch.equal(lg, again[0]) and torch.equal(iou, again[1])
    for j in range(3):
        one = m.mask_decoder.decode(emb, None, s["points"][:, j:j + 1], s["labels"][:, j:j + 1], s["mask_input"])
        assert torch.equal(one[0][:, 0], lg[:, j]) and torch.equal(one[1][:, 0], iou[:, j]), j
    # the per-image mask is the mask repeated per problem
    rep = m.mask_decoder.decode(emb, None, s["points"], s["labels"], s["mask_input"][:, None].expand(-1, 3, -1, -1))
    assert torch.equal(rep[0], lg) and torch.equal(rep[1], iou)


def test_refinement_loop_feeds_a_decode_its_own_logits(goldens, models):
    (base, _), m = goldens["g8"], models["g8"]
    emb = base["emb"].to(DEV)
    first = m.decode_masks(emb, base["boxes"], multimask=True)
    mask = first.as_mask_input()
    assert tuple(mask.shape) == (2, 1, 32, 32) and torch.equal(mask, first.best().low_res_logits[:, :, 0])
    click = torch.tensor([[[[40.0, 50.0]]], [[[60.0, 30.0]]]])
    second = m.decode_masks(emb, base["boxes"], points=click, point_labels=torch.ones((2, 1, 1), dtype=torch.int64), mask_input=mask)
    lg, iou = m.mask_decoder.decode(emb, base["boxes"], click, torch.ones((2, 1, 1), dtype=torch.int32), mask)
    assert torch.equal(second.low_res_logits, lg[:, :, :1]) and torch.equal(second.iou, iou[:, :, :1])
    x = base["image"].to(DEV)                                                   # segment = image_encoder + decode_masks, bit for bit
    a = m.segment(x, base["boxes"], points=click, point_labels=torch.ones((2, 1, 1), dtype=torch.int64))
    b = m.decode_masks(m.image_encoder(x), base["boxes"], points=click, point_labels=torch.ones((2, 1, 1), dtype=torch.int64))
    assert torch.equal(a.low_res_logits, b.low_res_logits) and torch.equal(a.iou, b.iou)


# ---- the handle: optional weights, sizes, the memory contract ----------------------------------------------------------------------
def test_the_optional_weights_are_a_second_enumeration_and_groups_are_whole_or_absent(goldens, models, box_only):
    from vdr import _lib
    (base, _), m = goldens["g8"], models["g8"]
    d = m.mask_decoder
    lib = d.lib
    opt = [lib.vdr_mask_decoder_prompt_weight_name(d.h, i).decode() for i in range(lib.vdr_mask_decoder_num_prompt_weights(d.h))]
    assert len(opt) == 13 and set(opt) == set(PR.prompt_shapes()) | {"prompt_encoder.point_embeddings.0.weight", "prompt_encoder.point_embeddings.1.weight"}
    assert lib.vdr_mask_decoder_prompt_weight_name(d.h, 13) is None and lib.vdr_mask_decoder_prompt_weight_name(d.h, -1) is None
    names = {lib.vdr_mask_decoder_weight_name(d.h, i).decode() for i in range(lib.vdr_mask_decoder_num_weights(d.h))}
    assert not names & set(opt)                                                 # the first enumeration did not grow
    assert lib.vdr_mask_decoder_prompt_support(d.h) == 3
    assert lib.vdr_mask_decoder_prompt_support(box_only.mask_decoder.h) == 0 and not box_only.mask_decoder.has_point_prompts and not box_only.mask_decoder.has_mask_prompt
    # sizes: equal to the old function at 7 tokens, growing with the tokens
    assert d.workspace_bytes(3, 7) == d.workspace_bytes(3) and d.workspace_bytes(3, 7) < d.workspace_bytes(3, 9) < d.workspace_bytes(3, 16)
    n = C.c_size_t()
    assert lib.vdr_mask_decoder_workspace_bytes_prompts(d.h, 3, 6, C.byref(n)) == 0 and n.value < d.workspace_bytes(3)
    # a handle of its own: a group given in part is refused at finalize, naming the missing tensor
    cfg = _lib.vdr_mask_decoder_config(grid=8, img=128, channels=256, heads=8, depth=2, mlp_dim=128, attention_downsample_rate=2, mask_tokens=4,
                                       upscale_channels_1=64, upscale_channels_2=32, iou_head_depth=3, ln_eps=1e-6, final_ln_eps=1e-5, ln2d_eps=1e-6)

    def build(extra):
        h = C.c_void_p()
        assert lib.vdr_mask_decoder_create(C.byref(cfg), 0, C.byref(h)) == 0
        required = [lib.vdr_mask_decoder_weight_name(h, i).decode() for i in range(lib.vdr_mask_decoder_num_weights(h))]
        for name in required + list(extra):
            t = base["weights"][name].float().contiguous()
            assert lib.vdr_mask_decoder_set_weight(h, name.encode(), t.data_ptr(), (C.c_int64 * t.dim())(*t.shape), t.dim()) == 0, name
        rc = lib.vdr_mask_decoder_finalize(h)
        err = lib.vdr_last_error(None)
        support = lib.vdr_mask_decoder_prompt_support(h)
        lib.vdr_mask_decoder_destroy(h)
        return rc, err, support
    assert build([])[::2] == (0, 0) and build(opt[:3])[::2] == (0, 1) and build(opt[3:])[::2] == (0, 2) and build(opt)[::2] == (0, 3)
    rc, err, _ = build(opt[:2])
    assert rc == -6 and b"prompt_encoder.not_a_point_embed.weight" in err      # VDR_ERR_INCOMPLETE
    rc, err, _ = build(opt[3:12])
    assert rc == -6 and b"prompt_encoder.mask_downscaling.6.bias" in err
    h = C.c_void_p()
    assert lib.vdr_mask_decoder_create(C.byref(cfg), 0, C.byref(h)) == 0
    bad = torch.zeros(5)
    assert lib.vdr_mask_decoder_set_weight(h, (PR.MD + "0.bias").encode(), bad.data_ptr(), (C.c_int64 * 1)(5), 1) == -1   # element count
    lib.vdr_mask_decoder_destroy(h)


def test_prompts_without_their_weights_are_refused_before_the_device_is_touched(goldens, box_only):
    from vdr import _lib
    base, _ = goldens["g8"]
    d = box_only.mask_decoder
    emb, boxes = base["emb"].to(DEV).contiguous(), base["boxes"].to(DEV).float().contiguous()
    pts, lbl = torch.zeros((2, 1, 1, 2), device=DEV), torch.ones((2, 1, 1), dtype=torch.int32, device=DEV)
    mask = torch.zeros((2, 32, 32), device=DEV)
    ws = torch.full((d.workspace_bytes(2, 8),), mg.CANARY, dtype=torch.uint8, device=DEV)
    for pr, T in ((_lib.vdr_mask_prompts(boxes=boxes.data_ptr(), points=pts.data_ptr(), labels=lbl.data_ptr(), points_per_problem=1), 8),
                  (_lib.vdr_mask_prompts(points=pts.data_ptr(), labels=lbl.data_ptr(), points_per_problem=1), 7),
                  (_lib.vdr_mask_prompts(boxes=boxes.data_ptr(), mask_input=mask.data_ptr()), 7)):
        rc, _, _, _ = _raw_decode(d, emb, pr, 2, 1, T, ws)
        assert rc == -7 and b"need" in d.lib.vdr_last_error(None)               # VDR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((ws == mg.CANARY).all())
    rc, lg, iou, _ = _raw_decode(d, emb, _lib.vdr_mask_prompts(boxes=boxes.data_ptr()), 2, 1, 7)   # boxes alone still decode
    want = d.decode(emb, base["boxes"])
    assert rc == 0 and torch.equal(lg, want[0]) and torch.equal(iou, want[1])
    with pytest.raises(ValueError, match="weights absent"):
        box_only.decode_masks(emb, points=pts.cpu(), point_labels=lbl.cpu())
    with pytest.raises(ValueError, match="weights absent"):
        box_only.decode_masks(emb, base["boxes"], mask_input=mask.cpu())


@pytest.mark.parametrize("kind", ["points", "box_points", "box_mask", "points_mask_per_image"])
def test_decode_memory_contract_with_every_prompt_kind(goldens, models, kind):
    """test_decode_memory_contract's statement for vdr_mask_decode_prompts: a workspace one byte short is refused with nothing
    written; in a workspace of exactly the stated size the decode gives the bits of any other decode and touches no byte past
    it, nor around its outputs"""
    from vdr import _lib
    (base, sets), m = goldens["g10"], models["g10"]
    d = m.mask_decoder
    by = {s["name"]: s for s in sets}
    s = {"points": by["points3"], "box_points": by["box_points2"], "box_mask": by["box_refine"], "points_mask_per_image": by["points10_mask"]}[kind]
    emb = base["emb"].to(DEV).contiguous()
    B, nb, g = 1, 3, d.g
    P = B * nb
    keep = [t if t is None else t.to(DEV).contiguous() for t in (s["boxes"], s["points"], s["labels"], s["mask_input"])]
    bx, pt, lb, mk = keep
    npts = 0 if pt is None else pt.shape[2]
    T = 5 + npts + (2 if bx is not None else 1)
    pr = _lib.vdr_mask_prompts(boxes=None if bx is None else bx.data_ptr(), points=None if pt is None else pt.data_ptr(),
                               labels=None if lb is None else lb.data_ptr(), points_per_problem=npts,
                               mask_input=None if mk is None else mk.data_ptr(), mask_per_image=int(mk is not None))
    need = d.workspace_bytes(P, T)
    whole, body = mg.guarded(need, 4096)
    lw, lbody = mg.guarded(P * 4 * 16 * g * g * 4, 4096)
    iw, ib = mg.guarded(P * 4 * 4, 4096)

    def call(nbytes):
        return d.lib.vdr_mask_decode_prompts(d.h, emb.data_ptr(), 0, C.byref(pr), B, nb, body.data_ptr(), nbytes, lbody.data_ptr(), ib.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
    assert call(need - 1) == -5 and b"workspace too small" in d.lib.vdr_last_error(None)
    torch.cuda.synchronize()
    for t in (whole, lw, iw):
        assert bool((t == mg.CANARY).all())                                     # nothing written anywhere
    assert call(need) == 0
    torch.cuda.synchronize()
    assert mg.guards_intact(whole, 4096) and mg.guards_intact(lw, 4096) and mg.guards_intact(iw, 4096)
    lg, iou = d.decode(emb, s["boxes"], s["points"], s["labels"], s["mask_input"])
    assert torch.equal(lbody.view(torch.float32).view(lg.shape), lg) and torch.equal(ib.view(torch.float32).view(iou.shape), iou)
    assert mg.canary_left(lbody.view(torch.float32)) == 0 and mg.canary_left(ib.view(torch.float32)) == 0
    lg2, iou2 = d.decode(emb.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), s["boxes"], s["points"], s["labels"], s["mask_input"])
    assert torch.equal(lg2, lg) and torch.equal(iou2, iou)                      # the channel-last embedding, read in place


# ---- the volume sweep ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume(goldens):
    base, _ = goldens["g8"]
    x = torch.cat([base["image"], base["image"].flip(-1), base["image"][:1].flip(-2)], dim=0).to(DEV)   # Z = 5 slices [5, 3, 128, 128]
    return x, torch.tensor([20.0, 30.0, 90.0, 100.0])


def _emb(m, x, max_batch):
    """the embeddings as propagate_masks computes them: the encoder in chunks of max_batch (its bits may depend on the batch)"""
    return torch.cat([m.image_encoder(x[s0:s0 + max_batch]) for s0 in range(0, x.shape[0], max_batch)], dim=0)


def _hand_loop(m, x, box, index, order, margin, use_mask, max_batch=16):
    """decode_masks + the torch statement of mask_box, slice by slice"""
    emb = _emb(m, x, max_batch)
    out = {}
    seg = m.decode_masks(emb[index:index + 1], box.reshape(1, 1, 4))
    state = (seg.low_res_logits[0, 0, 0], box.to(DEV).float())
    for z in [index] + list(order):
        if z != index:
            seg = m.decode_masks(emb[z:z + 1], state[1].reshape(1, 1, 4), mask_input=state[0].reshape(1, 1, *state[0].shape) if use_mask else None)
        used = box.to(DEV).float() if z == index else state[1]
        lg = seg.low_res_logits[0, 0, 0]
        nxt, area = PR.mask_box_ref(lg[None], used[None], m.cfg.img, margin, 0.0)
        out[z] = (lg, seg.iou[0, 0, 0], used, area[0])
        state = (lg, nxt[0])
    return out


@pytest.mark.parametrize("use_mask", [True, False])
def test_propagate_masks_equals_a_hand_loop_bit_for_bit(models, volume, use_mask):
    m, (x, box) = models["g8"], volume
    vol = m.propagate_masks(x, box, 2, direction="both", margin=8, use_mask_prompt=use_mask, max_batch=2)
    assert tuple(vol.low_res_logits.shape) == (5, 32, 32) and tuple(vol.iou.shape) == (5,) and tuple(vol.boxes.shape) == (5, 4) and vol.area.dtype == torch.int32
    want = dict(_hand_loop(m, x, box, 2, [3, 4], 8.0, use_mask, 2))
    want.update({z: v for z, v in _hand_loop(m, x, box, 2, [1, 0], 8.0, use_mask, 2).items() if z < 2})
    for z in range(5):
        lg, iou, used, area = want[z]
        assert torch.equal(vol.low_res_logits[z], lg) and torch.equal(vol.iou[z], iou), z
        assert torch.equal(vol.boxes[z], used) and int(vol.area[z]) == int(area), z
    up = m.propagate_masks(x, box, 2, direction="up", use_mask_prompt=use_mask, max_batch=2)
    down = m.propagate_masks(x, box, 2, direction="down", use_mask_prompt=use_mask, max_batch=2)
    assert torch.equal(up.low_res_logits[2:], vol.low_res_logits[2:]) and torch.equal(down.low_res_logits[:3], vol.low_res_logits[:3])
    assert torch.equal(up.boxes[2:], vol.boxes[2:]) and torch.equal(down.boxes[:3], vol.boxes[:3]) and torch.equal(up.area[2:], vol.area[2:])
    masks = vol.masks(size=(50, 70))
    assert tuple(masks.shape) == (5, 50, 70) and masks.dtype == torch.bool
    multi = m.propagate_masks(x, box, 2, use_mask_prompt=use_mask, multimask=True, max_batch=2)   # the stored mask changes, the sweep does not
    assert torch.equal(multi.boxes, vol.boxes) and torch.equal(multi.area, vol.area)
    best = m.decode_masks(_emb(m, x, 2)[2:3], box.reshape(1, 1, 4), multimask=True).best()
    assert torch.equal(multi.low_res_logits[2], best.low_res_logits[0, 0, 0]) and torch.equal(multi.iou[2], best.iou[0, 0, 0])


def test_box_only_propagation_runs_without_mask_weights_and_an_empty_seed_keeps_its_box(goldens, box_only, volume):
    x, box = volume
    with pytest.raises(ValueError, match="weights absent"):
        box_only.propagate_masks(x, box, 0)
    # (encoder chunks of 2, as everywhere in this file: the comparison needs the two encoder runs to give the same bits)
    vol = box_only.propagate_masks(x, box, 0, use_mask_prompt=False, max_batch=2)
    want = _hand_loop(box_only, x, box, 0, [1, 2, 3, 4], 8.0, False, 2)
    for z in range(5):
        assert torch.equal(vol.low_res_logits[z], want[z][0]) and torch.equal(vol.boxes[z], want[z][2]), z
    # a decoder whose single-mask logits are all negative: the second transposed convolution is zero with bias 8 (the device
    # GELU gives gelu(8) = 8 exactly), mask token 0's hypernetwork ends in weight 0 and bias -1: every logit is 32 * (-8) = -256
    base, _ = goldens["g8"]
    w = dict(base["weights"])
    w["mask_decoder.output_upscaling.3.weight"] = torch.zeros_like(w["mask_decoder.output_upscaling.3.weight"])
    w["mask_decoder.output_upscaling.3.bias"] = torch.full_like(w["mask_decoder.output_upscaling.3.bias"], 8.0)
    w["mask_decoder.output_hypernetworks_mlps.0.layers.2.weight"] = torch.zeros_like(w["mask_decoder.output_hypernetworks_mlps.0.layers.2.weight"])
    w["mask_decoder.output_hypernetworks_mlps.0.layers.2.bias"] = torch.full_like(w["mask_decoder.output_hypernetworks_mlps.0.layers.2.bias"], -1.0)
    with _model({**base, "weights": w}, "sam_prompts_negative") as neg:
        vol = neg.propagate_masks(x, box, 2, max_batch=2)
        torch.cuda.synchronize()
        assert bool((vol.low_res_logits == -256.0).all()) and vol.area.tolist() == [0] * 5
        assert torch.equal(vol.boxes, box.to(DEV)[None].expand(5, -1)) and not bool(vol.masks().any())


def test_propagate_segmentation_returns_the_mask_generate_features_takes(models):
    import vdr
    m = models["g8"]
    H, W, S = 96, 80, 5
    vol = torch.rand((H, W, S), generator=torch.Generator().manual_seed(71)).numpy().astype(np.float32)
    box = np.array([20.0, 25.0, 60.0, 70.0])
    mask = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2)
    assert mask.shape == (H, W, S) and mask.dtype == np.bool_
    assert np.array_equal(mask, vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=2))
    # slice `index` is segment_slice's mask of the same box (chunks of one: the same encoder batch, the same decode)
    alone = vdr.pipeline.propagate_segmentation(m, vol, box, 2, max_batch=1)
    assert np.array_equal(alone[:, :, 2], vdr.segment_slice(m, vol[:, :, 2], box))
    one = vdr.segment_slice(m, vol[:, :, 2], box, points=[[40.0, 50.0]], point_labels=[1])
    assert one.shape == (H, W) and one.dtype == np.bool_
    if not mask.any():                                                          # (random weights: any mask will do for the plumbing)
        mask[30:50, 30:50, :] = True
    feats, masks = vdr.pipeline.generate_features(m, vol, mask)
    assert len(feats) == S and len(masks) == S and feats[0].shape[-1] == 256
