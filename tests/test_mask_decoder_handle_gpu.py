"""GPU: the vdr_mask_decoder handle as an object -- what it enumerates, what it owns and where it runs.  Everything goes through
vdr.segment.MaskDecoder / the C ABI; the arithmetic of a decode is tests/test_sam_decoder_gpu.py's and tests/test_sam_prompts_gpu.py's.

1. Names: vdr_mask_decoder_weight_name and vdr_mask_decoder_prompt_weight_name, name by name and in order, against a record.
2. Reload and lifetime: decoders from other weights give other bits and none leaves anything behind for the next; a decoder
   with one optional group decodes that group's prompts like the full one; a group given in part is refused by finalize;
   handles destroyed with nothing set and after a refused finalize.
3. Memory: see test_destroyed_decoders_give_their_device_memory_back.
4. Device: see test_a_decoder_runs_on_its_own_device_and_leaves_the_current_one.

tests/ledger/mask_decoder_weight_names.json is a RECORD of the library at the commit its header names, never of the code under test:
    python tests/test_mask_decoder_handle_gpu.py --record tests/ledger/mask_decoder_weight_names.json --lib path/to/libvdr.so --commit <sha>
"""
import ctypes as C
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "ledger", "mask_decoder_weight_names.json")

if __name__ == "__main__":  # (--record: the paths tests/conftest.py sets up under pytest)
    for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "vit-deep-radiomics_amd"), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import sam_decoder_ref as R  # noqa: E402
import sam_prompt_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_INCOMPLETE = -6
MLP_DIMS = (128, 2048)
POINT_GROUP = ("prompt_encoder.point_embeddings.0.weight", "prompt_encoder.point_embeddings.1.weight", "prompt_encoder.not_a_point_embed.weight")


def _create(lib, grid, mlp_dim, device=0, img=128):
    from vdr import _lib
    cfg = _lib.vdr_mask_decoder_config(grid=grid, img=img, channels=256, heads=8, depth=2, mlp_dim=mlp_dim, attention_downsample_rate=2, mask_tokens=4,
                                       upscale_channels_1=64, upscale_channels_2=32, iou_head_depth=3, **R.SA_EPS)
    h = C.c_void_p()
    assert lib.vdr_mask_decoder_create(C.byref(cfg), device, C.byref(h)) == 0
    return h


def _enumerations(lib, h):
    return {"required": [lib.vdr_mask_decoder_weight_name(h, i).decode() for i in range(lib.vdr_mask_decoder_num_weights(h))],
            "prompt": [lib.vdr_mask_decoder_prompt_weight_name(h, i).decode() for i in range(lib.vdr_mask_decoder_num_prompt_weights(h))]}


def _names(mlp_dim):
    from vdr import _lib
    lib = _lib.load()
    h = _create(lib, 8, mlp_dim)
    try:
        return _enumerations(lib, h)
    finally:
        lib.vdr_mask_decoder_destroy(h)


# ---- 1. names ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_the_record_holds_both_sizes_and_they_agree(record):
    assert sorted(record["configs"]) == sorted(f"mlp_dim_{m}" for m in MLP_DIMS)
    assert len(record["recorded_at_commit"]) == 40
    assert record["configs"]["mlp_dim_128"] == record["configs"]["mlp_dim_2048"]


@pytest.mark.parametrize("mlp_dim", MLP_DIMS)
def test_both_enumerations_match_the_record(record, mlp_dim):
    got, want = _names(mlp_dim), record["configs"][f"mlp_dim_{mlp_dim}"]
    print(f"mlp_dim {mlp_dim}: {len(got['required'])} required and {len(got['prompt'])} prompt names, record {len(want['required'])} and {len(want['prompt'])}")
    assert got["required"] == want["required"] and got["prompt"] == want["prompt"]
    assert tuple(got["prompt"][:3]) == POINT_GROUP and all(n.startswith(PR.MD) for n in got["prompt"][3:])


# ---- 2. reload and lifetime ---------------------------------------------------------------------------------------------------------
G, IMG = 8, 128


@pytest.fixture(scope="module")
def case():
    """one embedding and two boxes (P = 2); two points per problem and one mask per problem for the prompt decodes"""
    gen = torch.Generator().manual_seed(11)
    return dict(emb=torch.randn((1, 256, G, G), generator=gen).cuda(), boxes=torch.tensor([[[10.0, 20.0, 90.0, 100.0], [33.0, 5.0, 120.0, 77.0]]]),
                points=torch.rand((1, 2, 2, 2), generator=gen) * IMG, labels=torch.tensor([[[1, 0], [1, 1]]], dtype=torch.int32),
                mask=torch.randn((1, 2, 4 * G, 4 * G), generator=gen) * 3)


def _decoder(w, grid=G, device="cuda:0"):
    from vdr.segment import MaskDecoder
    return MaskDecoder(w, grid, IMG, torch.device(device), **R.SA_EPS)


def _decode(d, case, **kw):
    out = d.decode(case["emb"].to(d.device), case["boxes"], **kw)
    torch.cuda.synchronize(d.device)
    return [t.cpu() for t in out]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def test_decoders_from_other_weights_leave_nothing_behind(case):
    wa, wb = PR.all_weights(3, 128, 4), PR.all_weights(33, 128, 44)
    outs = []
    for w in (wa, wb, wa):
        d = _decoder(w)
        outs.append(_decode(d, case) + _decode(d, case, points=case["points"], labels=case["labels"], mask_input=case["mask"]))
        d.__del__()
    assert _same(outs[0], outs[2]), "weights A again: the same bits"
    assert not any(torch.equal(p, q) for p, q in zip(outs[0], outs[1])), "weights B change every output"


def test_a_decoder_with_one_optional_group_decodes_like_the_full_one(case):
    w = PR.all_weights(3, 128, 4)
    full = _decoder(w)
    points_only = _decoder({k: v for k, v in w.items() if not k.startswith(PR.MD)})
    mask_only = _decoder({k: v for k, v in w.items() if k not in POINT_GROUP})
    lib = full.lib
    assert [lib.vdr_mask_decoder_prompt_support(d.h) for d in (full, points_only, mask_only)] == [3, 1, 2]
    pts, msk = dict(points=case["points"], labels=case["labels"]), dict(mask_input=case["mask"])
    assert _same(_decode(points_only, case, **pts), _decode(full, case, **pts))
    assert _same(_decode(mask_only, case, **msk), _decode(full, case, **msk))
    assert _same(_decode(points_only, case), _decode(full, case)) and _same(_decode(mask_only, case), _decode(full, case))


def _set(lib, h, w, names):
    for name in names:
        t = w[name].float().contiguous()
        assert lib.vdr_mask_decoder_set_weight(h, name.encode(), t.data_ptr(), (C.c_int64 * t.dim())(*t.shape), t.dim()) == 0, name


def test_refused_finalizes_and_empty_handles_destroy_cleanly(case):
    from vdr import _lib
    lib = _lib.load()
    w = PR.all_weights(3, 128, 4)
    want = None
    h = _create(lib, G, 128)
    names = _enumerations(lib, h)
    lib.vdr_mask_decoder_destroy(h)                                            # nothing set
    lib.vdr_mask_decoder_destroy(None)                                         # (a null handle is accepted)
    for given, missing in ((names["prompt"][:2], names["prompt"][2]), (names["prompt"][3:12], names["prompt"][12]),
                           (names["prompt"][:3] + names["prompt"][4:], names["prompt"][3])):
        h = _create(lib, G, 128)
        _set(lib, h, w, names["required"] + given)
        assert lib.vdr_mask_decoder_finalize(h) == ERR_INCOMPLETE
        err = lib.vdr_last_error(None)
        assert missing.encode() in err and b"given in part" in err
        assert lib.vdr_mask_decoder_prompt_support(h) == 0
        lib.vdr_mask_decoder_destroy(h)                                        # after a refused finalize
        got = _decode(_decoder(w), case)                                       # and a fresh decoder computes the same bits
        want = want or got
        assert _same(got, want)
    h = _create(lib, G, 128)
    _set(lib, h, w, names["required"][:-1])
    assert lib.vdr_mask_decoder_finalize(h) == ERR_INCOMPLETE and names["required"][-1].encode() in lib.vdr_last_error(None)
    lib.vdr_mask_decoder_destroy(h)


# ---- 3. memory --------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_destroyed_decoders_give_their_device_memory_back():
    """Six cycles of: create, set every weight, finalize, one decode, destroy, at grid 32 and mlp_dim 2048 (about 8 MiB of bf16
    matrices and 2.5 MiB of positional tables per decoder).  Cycle 1 warms up torch's allocator and the runtime.  With F = free
    device memory just before cycle 2's create minus just after its finalize, and drift = free memory after cycle 2's destroy
    minus after cycle 6's, the test asserts drift <= F / 8: over four cycles that catches anything of F / 32 or more a destroyed
    decoder keeps.  F > 4 MiB only says that the footprint shows in mem_get_info at all: 12 MiB as measured (one arena of
    10.5 MiB).  On the library before the arena, whose ~110 allocations of at most 1 MiB came out of memory the runtime keeps,
    F read 0 and this guard alone failed; drift was 0 there too (profiles/mask_decoder_handle_refactor_ab.txt)."""
    w = PR.all_weights(3, 2048, 4)
    gen = torch.Generator().manual_seed(12)
    case = dict(emb=torch.randn((1, 256, 32, 32), generator=gen).cuda(), boxes=torch.tensor([[[10.0, 20.0, 90.0, 100.0]]]))
    F, after_close, outs = None, {}, {}
    for cycle in range(1, 7):
        before = _free_bytes()
        d = _decoder(w, grid=32)
        if cycle == 2:
            F = before - _free_bytes()
        outs[cycle] = _decode(d, case)
        d.__del__()
        del d
        after_close[cycle] = _free_bytes()
    drift = after_close[2] - after_close[6]
    print(f"mask decoder g 32 mlp_dim 2048: F = {F} bytes ({F / 2**20:.2f} MiB), drift over cycles 3..6 = {drift} bytes ({drift / 2**20:.3f} MiB), "
          f"free after each destroy: {[after_close[c] for c in sorted(after_close)]}")
    assert _same(outs[2], outs[6])
    assert F > 4 * 2**20, "the decoder's footprint shows in mem_get_info"
    assert drift <= F / 8


# ---- 4. device ----------------------------------------------------------------------------------------------------------------------
def test_a_decoder_runs_on_its_own_device_and_leaves_the_current_one(case):
    """include/vdr.h: a handle's calls run on the handle's device whatever device is current, and leave the caller's current
    device unchanged.  With device 0 current, a decoder of device 1 is created, finalized and decodes tensors of device 1; the
    current device is 0 after each call and the bits are a device-0 decoder's.  (The only case of this file that is expected to
    fail on the library before the decoder was bound to its device: its create left device 1 current and its decode ran on the
    current one.)"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    from vdr import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    w = PR.all_weights(3, 128, 4)
    h = _create(lib, G, 128, device=1)
    assert torch.cuda.current_device() == 0
    lib.vdr_mask_decoder_destroy(h)
    assert torch.cuda.current_device() == 0
    d1 = _decoder(w, device="cuda:1")                                          # create, set_weight, finalize
    assert torch.cuda.current_device() == 0
    kw = dict(points=case["points"], labels=case["labels"], mask_input=case["mask"])
    got = _decode(d1, case) + _decode(d1, case, **kw)
    assert torch.cuda.current_device() == 0
    d0 = _decoder(w)
    assert _same(got, _decode(d0, case) + _decode(d0, case, **kw))
    d1.__del__()
    assert torch.cuda.current_device() == 0


def _record(argv):
    import argparse
    ap = argparse.ArgumentParser(description="record the mask decoder's two name enumerations from a build of libvdr.so")
    ap.add_argument("--record", required=True, metavar="NAMES.json")
    ap.add_argument("--lib", help="the libvdr.so to record from (default: the package's own)")
    ap.add_argument("--commit", required=True, help="the commit that library was built at (the record's header)")
    a = ap.parse_args(argv)
    from vdr import _lib as L
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)  # before the first load()
    out = {f"mlp_dim_{m}": _names(m) for m in MLP_DIMS}
    for name, e in out.items():
        print(name, len(e["required"]), len(e["prompt"]), flush=True)
    with open(a.record, "w") as f:
        json.dump({"recorded_at_commit": a.commit, "configs": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    _record(sys.argv[1:])
