"""GPU: the lifetime of a vdr_handle -- weights reloaded into a live handle, error paths that end in vdr_destroy, and device
memory that comes back when a handle is destroyed.  Everything goes through Engine / the C ABI.

1. Reload: weights A, then B (another seed), then A again give y_A, y_B != y_A and y_A again BIT FOR BIT, so every copy
   vdr_finalize derives from the loaded weights (LayerNorm-folded weights and their column sums, MX-fp8 payloads and scales,
   pair-interleaved GEMM operands, the packed rel-pos operand, resampled SAM tables, the position and RoPE tables of the
   input size in force) is rebuilt from the new weights and none is left stale.
2. Error paths: a handle destroyed with nothing set, after a refused vdr_finalize, after a weight set twice, after a
   refused vdr_set_input_size -- each returns its documented code and a fresh handle afterwards computes the same bits.
3. Memory: see test_destroyed_handles_give_their_device_memory_back.
"""
import ctypes as C

import pytest
import torch

from handle_configs import P16, POSTLN, SAM, SWIGLU, reg_cfg, sam_config, sized_sam, vit_config
from oracle import sam_oracle as so
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_INCOMPLETE, ERR_UNSUPPORTED = -1, -6, -7


def _forwards(e, x, modes):
    out = [e.forward(x, m) for m in modes]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 1. reload ----------------------------------------------------------------------------------------------------------------
def _vit_case(cfg, batch, **kw):
    def make():
        import vdr
        e = vdr.Engine(vit_config(cfg, **kw))
        return (e, vo.make_weights(cfg, seed=3, scale=0.05), vo.make_weights(cfg, seed=33, scale=0.05),
                vo.make_images(cfg, batch, seed=4).cuda(), (vdr.OUT_TOKENS, vdr.OUT_CLS))
    return make


def _sam_case(native_tables):
    def make():
        import vdr
        # native_tables: a handle built at 96^2 (grid 6: padded windows); A carries pos_embed [1, 10, 10, D] and the global
        # block's rel_pos [19, 64] of the 160^2 checkpoint (kept as loaded, resampled by vdr_finalize), B the handle's own shapes
        cs = sized_sam(SAM, 96) if native_tables else SAM
        e = vdr.Engine(sam_config(cs))
        return (e, so.make_weights(SAM, seed=21, scale=0.05), so.make_weights(cs, seed=22, scale=0.05),
                so.make_images(cs, 2, seed=23).cuda(), (vdr.OUT_ENCODER, vdr.OUT_TOKENS))
    return make


RELOAD_CASES = {
    "p16_d128-fold": _vit_case(P16, 5),
    "p16_d128-nofold": _vit_case(P16, 5, ln_fold=False),
    "dinov2_swiglu_ls-fp8_cls_bf16-streams2": _vit_case(SWIGLU, 5, fp8=1, fp8_cls_bf16=True, streams=2),
    "sam": _sam_case(False),
    "sam-native_tables": _sam_case(True),
}


@pytest.mark.parametrize("case", sorted(RELOAD_CASES))
def test_reloaded_weights_replace_every_derived_copy(case):
    e, wa, wb, x, modes = RELOAD_CASES[case]()
    e.load_weights(wa)
    ya = _forwards(e, x, modes)
    e.load_weights(wb)
    yb = _forwards(e, x, modes)
    assert not any(torch.equal(p, q) for p, q in zip(ya, yb)), "weights B change every output"
    e.load_weights(wa)
    assert _same(_forwards(e, x, modes), ya), "weights A again: the same bits"
    e.load_weights(wb)
    assert _same(_forwards(e, x, modes), yb), "weights B again: the same bits"
    e.close()


@pytest.mark.parametrize("name", ["dinov2reg_hf_tiny", "dinov3_hf_tiny"])
def test_reloaded_weights_rebuild_the_tables_of_the_size_in_force(name):
    """Register-token models (their position table is always a built one; DINOv3: RoPE tables): the weights are replaced
    while ANOTHER input size is in force, and the handle goes back to the native size afterwards."""
    import vdr
    import dinov3_ref as dr
    rc = reg_cfg(name)
    img = rc.vit.img
    e = vdr.Engine(dr.vdr_config(rc))
    wa, wb = dr.make_weights(rc, seed=5), dr.make_weights(rc, seed=55)
    x = vo.make_images(rc.vit, 3, seed=6).cuda()
    x2 = torch.rand(3, 3, 2 * img, img, generator=torch.Generator().manual_seed(7)).cuda()
    modes = (vdr.OUT_TOKENS, vdr.OUT_CLS)

    def both():  # ends at the 2:1 size
        e.set_input_size(img, img)
        native = _forwards(e, x, modes)
        e.set_input_size(2 * img, img)
        return native, _forwards(e, x2, modes)

    e.load_weights(wa)
    ya, ya2 = both()
    e.load_weights(wb)  # at the 2:1 size
    assert not any(torch.equal(p, q) for p, q in zip(ya2, _forwards(e, x2, modes)))
    yb, yb2 = both()
    assert not any(torch.equal(p, q) for p, q in zip(ya, yb))
    e.load_weights(wa)  # at the 2:1 size again
    assert _same(_forwards(e, x2, modes), ya2)
    got, got2 = both()
    assert _same(got, ya) and _same(got2, ya2)
    e.close()


# ---- 2. error paths -------------------------------------------------------------------------------------------------------------
def _set_weight(e, name, t):
    a = t.detach().to("cpu", torch.float32).contiguous().numpy()
    shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
    return e.lib.vdr_set_weight(e.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, max(a.ndim, 1))


@pytest.fixture(scope="module")
def p16():
    """(weights, images, the tokens a fresh handle computes)"""
    import vdr
    w = vo.make_weights(P16, seed=3, scale=0.05)
    x = vo.make_images(P16, 5, seed=4).cuda()
    e = vdr.Engine(vit_config(P16))
    e.load_weights(w)
    y = _forwards(e, x, (vdr.OUT_TOKENS,))
    e.close()
    return w, x, y


def _fresh_handle_works(p16):
    import vdr
    w, x, y = p16
    e = vdr.Engine(vit_config(P16))
    e.load_weights(w)
    assert _same(_forwards(e, x, (vdr.OUT_TOKENS,)), y)
    e.close()


def test_destroy_with_nothing_set(p16):
    import vdr
    e = vdr.Engine(vit_config(P16))
    e.close()
    e.lib.vdr_destroy(None)  # (a null handle is accepted)
    _fresh_handle_works(p16)


def test_finalize_with_a_weight_missing_then_destroy(p16):
    import vdr
    w = p16[0]
    e = vdr.Engine(vit_config(P16))
    names = e.weight_names()
    missing = "blocks.1.mlp.fc1.weight"
    assert missing in names
    for n in names:
        if n != missing:
            assert _set_weight(e, n, w[n]) == 0, n
    assert e.lib.vdr_finalize(e.h) == ERR_INCOMPLETE
    assert missing.encode() in e.lib.vdr_last_error(e.h)
    e.close()
    _fresh_handle_works(p16)


def test_a_weight_set_twice(p16):
    import vdr
    w, x, y = p16
    e = vdr.Engine(vit_config(P16))
    for n in e.weight_names():
        assert _set_weight(e, n, torch.zeros_like(w[n])) == 0, n  # first zeros ...
        assert _set_weight(e, n, w[n]) == 0, n                    # ... then the weight: the second call wins
    assert _set_weight(e, "blocks.0.norm1.weight", torch.zeros(P16.dim + 1)) == ERR_INVALID  # (and a refused one changes nothing)
    assert e.lib.vdr_finalize(e.h) == 0
    assert _same(_forwards(e, x, (vdr.OUT_TOKENS,)), y)
    e.close()
    _fresh_handle_works(p16)


def test_set_input_size_refused_on_a_token_model(p16):
    import vdr
    e = vdr.Engine(vit_config(POSTLN))
    e.load_weights(vo.make_weights(POSTLN, seed=13, scale=0.05))
    assert e.lib.vdr_set_input_size(e.h, 64, 64) == ERR_UNSUPPORTED
    assert b"token model" in e.lib.vdr_last_error(e.h)
    t = vo.make_tokens(4, 17, POSTLN.dim, seed=14).cuda()
    y = e.forward_tokens(t, vdr.OUT_CLS)
    assert torch.isfinite(y).all()  # the handle is still good
    e.close()
    _fresh_handle_works(p16)


# ---- 3. memory --------------------------------------------------------------------------------------------------------------------
BIG = vo.VitCfg(64, 16, 3, 512, 8, 2, 2048)  # ~6 MB of bf16 weights per block


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("variant", ["fold", "fp8_cls_bf16-streams2"])
def test_destroyed_handles_give_their_device_memory_back(variant):
    """Six cycles of: create, load, one forward at batch 4, (bf16 handle) set_input_size(128, 128) and back, reload the
    weights, destroy.  The config's device footprint (60-72 MiB per handle as mem_get_info reports it: the bf16 weights,
    their folded or fp8 copies, the interleaved copies, the counter array) dwarfs any allocation granule.  Cycle 1 warms up
    torch's allocator and the runtime.  With F = free device memory just before cycle 2's create minus just after its
    finalize, and drift = free memory after cycle 2's destroy minus after cycle 6's, the test asserts drift <= F / 8: over
    four cycles that catches any class of buffer of F / 32 (about 2 MiB at the measured F) or more that a destroyed handle
    keeps -- the copies of the qkv / fc1 / fc2 weights (1.5 to 4 MiB each, several per handle), the fp8 payloads.  It does NOT see the small
    buffers (column sums and folded biases, position / RoPE / rel-pos tables, scales, streams, events):
    their safety is structural -- every device buffer, stream and event of a handle is a member that frees itself, and
    vdr_destroy is `delete`.  The forwards of cycle 2 and cycle 6 are compared bit for bit as well."""
    import vdr
    kw = {} if variant == "fold" else dict(fp8=1, fp8_cls_bf16=True, streams=2)
    w = vo.make_weights(BIG, seed=3, scale=0.05)
    x = vo.make_images(BIG, 4, seed=4).cuda()
    x2 = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    F, after_close, outs = None, {}, {}
    for cycle in range(1, 7):
        before = _free_bytes()
        e = vdr.Engine(vit_config(BIG, **kw))
        e.load_weights(w)
        if cycle == 2:
            F = before - _free_bytes()
        y = [e.forward(x, vdr.OUT_TOKENS)]
        if not kw:
            e.set_input_size(128, 128)
            y.append(e.forward(x2, vdr.OUT_TOKENS))
            e.set_input_size(64, 64)
        e.load_weights(w)
        y.append(e.forward(x, vdr.OUT_CLS))
        outs[cycle] = [t.cpu() for t in y]
        del y
        e.close()
        del e
        after_close[cycle] = _free_bytes()
    drift = after_close[2] - after_close[6]
    print(f"{variant}: F = {F} bytes ({F / 2**20:.2f} MiB), drift over cycles 3..6 = {drift} bytes ({drift / 2**20:.3f} MiB), "
          f"free after each destroy: {[after_close[c] for c in sorted(after_close)]}")
    assert _same(outs[2], outs[6])
    assert F > 16 * 2**20, "the handle's footprint shows in mem_get_info"
    assert drift <= F / 8
