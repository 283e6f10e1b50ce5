"""GPU: the launch ledger -- what every kind of forward enqueues, as the library's own profiler books it.

vdr_api.hip runs the transformer blocks of every model through one loop whose path-dependent steps (MX-fp8, folded
LayerNorm, explicit LayerNorm pre- / post-LN) are chosen once per call.  Nothing else in the suite pins the launch
SEQUENCE of a forward: outputs can stay inside their gates while a launch is added, dropped or booked under another class.
For each case of tests/forward_cases.py one forward runs with Engine.profile(True) and profile_read() is compared with
tests/ledger/forward_launch_ledger.json for every kernel class: `launches` equal, `flops` and `bytes` equal (the same
doubles summed in the same order: rel 1e-12 is the JSON round trip, nothing else).

The ledger is a RECORD of the library at the commit its header names, never of the code under test:
    python tests/test_launch_ledger_gpu.py --record tests/ledger/forward_launch_ledger.json --lib path/to/libvdr.so --commit <sha>
(--hashes FILE also writes a sha256 per output tensor, for a one-off bitwise A/B of two builds).  A change that means to
alter what a forward launches re-records it from the build that change is compared against and says so.

The cases are the smallest shapes that reach each branch of the block loop, the CLS tail, the CLS rows' bf16 MLP and
the SAM loop; the one large case (ViT-B width, two blocks, batch 100) is the smallest launch at which the 8-phase qkv /
fc1 engage (M = 19 700: 77 x 9 = 693 and 77 x 12 = 924 tiles of 256 x 256, at least 512 needed) and the statistics are
finalised by ln_finalize or by the producers instead of inside the consumer.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LEDGER = os.path.join(HERE, "ledger", "forward_launch_ledger.json")

if __name__ == "__main__":  # (--record: the paths tests/conftest.py sets up under pytest)
    for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "vit-deep-radiomics_amd"), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from forward_cases import CASE_IDS, cases  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(make):
    """One profiled forward of a case: ({class: {launches, flops, bytes}}, the output tensors)."""
    e, forward = make()
    e.profile(True)
    outs = forward()
    torch.cuda.synchronize()
    prof = e.profile_read()
    e.profile(False)
    return {k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in prof.items()}, outs


@pytest.fixture(scope="module")
def ledger():
    with open(LEDGER) as f:
        return json.load(f)


def test_the_ledger_holds_exactly_the_cases(ledger):
    assert sorted(ledger["cases"]) == sorted(CASE_IDS) == sorted(cases())
    assert len(ledger["recorded_at_commit"]) == 40


@pytest.mark.parametrize("case", CASE_IDS)
def test_forward_launches_match_the_ledger(ledger, case):
    got, _ = _run(cases()[case])
    want = ledger["cases"][case]
    for k in sorted(set(got) | set(want)):
        print(f"{case} {k}: got {got.get(k)}  ledger {want.get(k)}")
    assert sorted(got) == sorted(want), "kernel classes with launches"
    for k in sorted(want):
        assert got[k]["launches"] == want[k]["launches"], (case, k)
        assert got[k]["flops"] == pytest.approx(want[k]["flops"], rel=1e-12, abs=0.0), (case, k)
        assert got[k]["bytes"] == pytest.approx(want[k]["bytes"], rel=1e-12, abs=0.0), (case, k)


def _record(argv):
    import argparse
    ap = argparse.ArgumentParser(description="record the launch ledger from a build of libvdr.so")
    ap.add_argument("--record", required=True, metavar="LEDGER.json")
    ap.add_argument("--lib", help="the libvdr.so to record from (default: the package's own)")
    ap.add_argument("--commit", required=True, help="the commit that library was built at (the ledger's header)")
    ap.add_argument("--hashes", metavar="FILE", help="also write `case index sha256` of every output tensor")
    a = ap.parse_args(argv)
    from vdr import _lib as L
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)  # before the first load(): every Engine of this process uses it
    table, out, hashes = cases(), {}, []
    assert sorted(table) == sorted(CASE_IDS)
    for cid in CASE_IDS:
        out[cid], outs = _run(table[cid])
        for i, t in enumerate(outs):
            h = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
            hashes.append(f"{cid} {i} {h}")
        print(cid, {k: v["launches"] for k, v in out[cid].items()}, flush=True)
    with open(a.record, "w") as f:
        json.dump({"recorded_at_commit": a.commit, "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.hashes:
        with open(a.hashes, "w") as f:
            f.write("\n".join(hashes) + "\n")


if __name__ == "__main__":
    _record(sys.argv[1:])
