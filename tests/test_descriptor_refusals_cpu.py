"""CPU: every refusal of the eleven descriptor entry points recorded in tests/golden/descriptor_refusals.json (README_refusals.md:
taken from the library BEFORE their operand checks became check_desc_operand) comes back with the recorded
code and the recorded message, except for the messages whose wording the unification changed, listed below with their new
text.  Every row of the table is a refused call (the generator's condition, asserted again here), so nothing in this file can
launch a kernel on the host pointers it passes; the un-mutated baselines are called only where there is no GPU."""
import ctypes as C
import json
import os

import pytest
import torch

from fixtures import lib  # noqa: F401

# old text -> new text, without the "<op>: " both start with (the list of DESIGN.md §4.6q).  Conditions that two copies worded
# differently and now share one wording:
REWORDED = {
    "null x, work or bits": "null pointer",
    "null x, y, work, row_sim or row_idx": "null pointer",
    "null x, mean, whiten or d2": "null pointer",
    "pointers, rows (ld) and images (image_stride) must be 16-byte aligned": "pointers, rows (ld) and image_stride must be 16-byte aligned",
    "pointers, rows (ld), images and problems (the strides) must be 16-byte aligned": "pointers, rows (ld) and the strides must be 16-byte aligned",
    "pointers, rows (ldx, ldy) and pair strides must be 16-byte aligned": "pointers, rows (ldx and ldy) and the pair strides must be 16-byte aligned",
    "x, mean, whiten, rows (ld), images, problems and the model strides must be 16-byte aligned, d2 4-byte aligned":
        "pointers, rows (ld) and the strides must be 16-byte aligned",
}
# ... and the alignment an op still checks itself, because the shared check does not know the argument: by mutated argument
OWN_ALIGNMENT = {
    "active": "active must be 16-byte aligned",
    "col_sim": "col_sim and col_idx must be 16-byte aligned",
    "col_idx": "col_sim and col_idx must be 16-byte aligned",
    "mean_stride": "the model strides (mean_stride, whiten_stride) must be 16-byte aligned, d2 4-byte aligned",
    "whiten_stride": "the model strides (mean_stride, whiten_stride) must be 16-byte aligned, d2 4-byte aligned",
    "d2": "the model strides (mean_stride, whiten_stride) must be 16-byte aligned, d2 4-byte aligned",
}
INVALID, UNSUPPORTED, NO_DEVICE = -1, -7, -2


@pytest.fixture(scope="module")
def table(golden_dir):
    with open(os.path.join(golden_dir, "descriptor_refusals.json")) as f:
        return json.load(f)


def _aligned(n=4096):
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) & ~15


def _call(lib, op, args, p):
    def native(v):
        if isinstance(v, str):
            return float("nan") if v == "nan" else p + int(v[1:] or 0)
        return v

    code = getattr(lib, op)(*(native(v) for v in args.values()))
    return code, (lib.vdr_last_error(None) or b"").decode()


def expected_message(row):
    op, _, what = row["message"].partition(": ")
    own = [OWN_ALIGNMENT[a] for a in row["mutation"] if a in OWN_ALIGNMENT]
    if "aligned" in what and own:
        return f"{op}: {own[0]}"
    return f"{op}: {REWORDED.get(what, what)}"


def test_every_recorded_refusal_is_still_that_refusal(lib, table):
    keep, p = _aligned()
    ops = sorted(table["baselines"])
    assert len(ops) == 11 and len(table["rows"]) >= 400
    seen = set()
    for row in table["rows"]:
        assert row["code"] in (INVALID, UNSUPPORTED), row  # never replay a call that was not refused
        assert row["message"].startswith(row["op"][len("vdr_op_"):] + ": "), row
        args = dict(table["baselines"][row["op"]][row["dtype"]], **row["mutation"])
        code, msg = _call(lib, row["op"], args, p)
        assert code == row["code"], (row, code, msg)
        assert msg == expected_message(row), (row, msg)
        seen.add(row["message"].partition(": ")[2])
    assert set(REWORDED) <= seen  # (no stale entry in the list)
    both = [op for op in ops if len(table["baselines"][op]) == 2]
    assert len(both) == 6 and all(set(table["baselines"][op]) == {"f32", "bf16"} for op in both)


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the un-mutated calls would launch on host pointers")
def test_the_baselines_are_valid_calls(lib, table):
    keep, p = _aligned()
    for op, by_dtype in table["baselines"].items():
        for args in by_dtype.values():
            code, msg = _call(lib, op, args, p)
            assert code == NO_DEVICE and "no CPU path" in msg, (op, code, msg)
