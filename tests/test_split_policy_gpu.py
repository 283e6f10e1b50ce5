"""GPU: the default split of large batches (vdr_config.streams = 0 and micro_batch = 0; csrc/vdr_api.hip default_split).

With both options left at 0 the library decides per call: the whole batch on the caller's stream, or two parts on two
internal streams where that costs the 8-phase qkv / fc1 GEMMs no extra round of tiles.  ViT-B width (dim 768, hidden 3072,
197 tokens) on a 256-CU device: batch 100 has no admissible pair (neither half reaches two rounds of tiles), batch 200 runs
as 100 + 100 (6 + 8 rounds either way), batch 256 as 146 + 110 (7 + 10 rounds; 128 + 128 would run 8 + 10).

What is held here: which batches split and into what (vdr_batch_plan and the profiler's launch counts against an engine
with streams = 1), that the bits do not change, that vdr_workspace_bytes covers what the split forward touches and one
byte less is refused with nothing written, that an explicit micro_batch / streams still means what it said, and that a
captured forward works.  The profiler sums a class over its launches, so the two parts cannot be read apart from it: the
parts' sizes come from vdr_batch_plan, and the class FLOPs of the split forward are held to those of a 146-image plus a
110-image forward on the one-stream engine.

Two blocks, seeded weights and images of oracle/vit_oracle.py, made once per module.
"""
import ctypes as C

import pytest
import torch

import handle_configs as hc
import memguard as mg
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

VITB2 = vo.VitCfg(224, 16, 3, 768, 12, 2, 3072)
PER_BLOCK = ("gemm_qkv", "attention", "gemm_proj", "gemm_fc1", "gemm_fc2")
GUARD = 4 << 20
VDR_ERR_WORKSPACE = -5


@pytest.fixture(scope="module")
def world():
    import vdr
    w = vo.make_weights(VITB2, seed=71)
    x = vo.make_images(VITB2, 256, seed=72).to(torch.bfloat16).cuda()
    engines = {"default": hc.engine(VITB2, w), "one": hc.engine(VITB2, w, streams=1),
               "halves": hc.engine(VITB2, w, micro_batch=128, streams=2)}
    ref = {}

    def reference(batch, mode):
        """the one-stream engine's output and profile for images [0, batch): computed once, never changed"""
        if (batch, mode) not in ref:
            out, prof = _profiled(engines["one"], x[:batch], mode)
            ref[batch, mode] = (out.clone(), prof)
        return ref[batch, mode]
    yield vdr, engines, x, reference
    for e in engines.values():
        e.close()


def _profiled(e, x, mode):
    e.profile(True)
    e.profile_read()
    out = e.forward(x, mode)
    torch.cuda.synchronize()
    prof = e.profile_read()
    e.profile(False)
    return out, prof


def _launches(prof):
    return {k: v["launches"] for k, v in prof.items()}


def test_batch_100_runs_whole_on_the_callers_stream(world):
    vdr, engines, x, reference = world
    assert engines["default"].batch_plan(100) == (100, 1, 1)
    want, prof_one = reference(100, vdr.OUT_CLS)
    got, prof = _profiled(engines["default"], x[:100], vdr.OUT_CLS)
    assert _launches(prof) == _launches(prof_one)
    assert torch.equal(got, want)


def test_batches_whose_last_rounds_are_nearly_full_stay_whole(world):
    """384: qkv 10.41 of 11 rounds, fc1 13.88 of 14 -- 0.71 of a round idle, below the 0.75 the split has to win back
    (measured slower split: DESIGN 5); 512: 0.68."""
    vdr, engines, x, reference = world
    assert engines["default"].batch_plan(384) == (384, 1, 1)
    assert engines["default"].batch_plan(512) == (512, 1, 1)


@pytest.mark.parametrize("batch,first", [(200, 100), (256, 146)])
def test_large_batch_runs_as_two_parts_same_bits(world, batch, first):
    vdr, engines, x, reference = world
    assert engines["default"].batch_plan(batch) == (first, 2, 2)
    assert engines["one"].batch_plan(batch) == (batch, 1, 1)
    want, prof_one = reference(batch, vdr.OUT_CLS)
    got, prof = _profiled(engines["default"], x[:batch], vdr.OUT_CLS)
    for k in PER_BLOCK:
        assert prof[k]["launches"] == 2 * prof_one[k]["launches"], (k, _launches(prof), _launches(prof_one))
        assert prof[k]["flops"] == prof_one[k]["flops"], k  # (nothing dropped, nothing run twice)
    assert torch.equal(got, want)


def test_parts_of_256_are_146_and_110(world):
    """The FLOPs of every per-block class are those of a 146-image forward plus a 110-image forward: in the ratio 146 : 110."""
    vdr, engines, x, reference = world
    mb, parts, streams = engines["default"].batch_plan(256)
    assert (mb, 256 - mb, parts, streams) == (146, 110, 2, 2)
    _, prof = _profiled(engines["default"], x, vdr.OUT_CLS)
    _, p146 = reference(146, vdr.OUT_CLS)
    _, p110 = reference(110, vdr.OUT_CLS)
    for k in PER_BLOCK:
        assert p146[k]["flops"] * 110 == p110[k]["flops"] * 146, k
        assert prof[k]["flops"] == p146[k]["flops"] + p110[k]["flops"], k
        assert prof[k]["launches"] == p146[k]["launches"] + p110[k]["launches"], k


def test_dense_output_at_200_same_bits(world):
    vdr, engines, x, reference = world
    want, _ = reference(200, vdr.OUT_DENSE)
    assert torch.equal(engines["default"].forward(x[:200], vdr.OUT_DENSE), want)


def test_explicit_halves_stay_halves(world):
    vdr, engines, x, reference = world
    assert engines["halves"].batch_plan(256) == (128, 2, 2)
    want, prof_one = reference(256, vdr.OUT_CLS)
    got, prof = _profiled(engines["halves"], x, vdr.OUT_CLS)
    for k in PER_BLOCK:
        assert prof[k]["launches"] == 2 * prof_one[k]["launches"], k
    assert torch.equal(got, want)


def _need(e, batch):
    need = C.c_size_t()
    assert e.lib.vdr_workspace_bytes(e.h, batch, 0, C.byref(need)) == 0
    return need.value


def test_workspace_bytes_covers_the_split_forward(world):
    """The forward at batch 256 in a body of exactly vdr_workspace_bytes between canary guards, prefilled with NaN bits:
    the guards keep every byte and the output is the one-stream engine's."""
    vdr, engines, x, reference = world
    e = engines["default"]
    want, _ = reference(256, vdr.OUT_CLS)
    whole, body = mg.guarded(_need(e, 256), GUARD)
    mg.fill(body, "ones")
    e._workspace = lambda batch, seq=0: body
    try:
        got = e.forward(x, vdr.OUT_CLS)
        torch.cuda.synchronize()
    finally:
        del e._workspace
    assert mg.guard_damage(whole, GUARD) == (None, None)
    assert torch.equal(got, want)


def test_workspace_one_byte_short_is_refused_and_untouched(world):
    vdr, engines, x, reference = world
    e = engines["default"]
    whole, body = mg.guarded(_need(e, 256) - 1, GUARD)
    out = torch.full((256, VITB2.dim), float("nan"), device="cuda")
    e._workspace = lambda batch, seq=0: body
    try:
        with pytest.raises(vdr.VdrError) as err:
            e.forward_into(x, out, vdr.OUT_CLS)
    finally:
        del e._workspace
    assert err.value.code == VDR_ERR_WORKSPACE, err.value
    torch.cuda.synchronize()
    assert bool((whole == mg.CANARY).all()) and bool(out.isnan().all())


def test_captured_forward_at_a_split_batch_replays_the_same_bits(world):
    """On a stream that is being captured the default split stays out (a captured forward is a linear graph); the
    workspace sized by vdr_workspace_bytes holds that form too."""
    vdr, engines, x, reference = world
    e = engines["default"]
    want, _ = reference(200, vdr.OUT_CLS)
    xs = x[:200]
    out = torch.empty((200, VITB2.dim), dtype=torch.float32, device="cuda")
    e._workspace(200)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            e.forward_into(xs, out, vdr.OUT_CLS)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
