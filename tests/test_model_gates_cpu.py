"""CPU: the model-level parity gate and the batch-property check of tests/model_gates.py reject what they are meant to
reject, each with a message that names the condition -- on plain torch tensors, nothing launched anywhere."""
import math

import pytest
import torch

from model_gates import check_batch_properties, check_parity, check_parity_fp8, gate_l2, gate_l2_fp8, min_cos, rel_l2

ROWS, COLS = 4096, 16
GATE = gate_l2(12)


@pytest.fixture(scope="module")
def ref():
    return torch.randn(ROWS, COLS, generator=torch.Generator().manual_seed(0))


def _rotate_row(t, row, cos):
    """t with one row turned, in its plane with a fixed direction and at its own length, to the given cosine with itself"""
    u = t[row].double()
    v = torch.ones(COLS, dtype=torch.float64)
    v = v - (v @ u) / (u @ u) * u
    v = v / v.norm() * u.norm()
    out = t.clone()
    out[row] = (cos * u + math.sqrt(1 - cos * cos) * v).float()
    return out


@pytest.mark.parametrize("layers", [0, 1, 12, 24, 40])
def test_gates_are_the_stated_formulas(layers):
    assert gate_l2(layers) == 4e-3 + 3e-3 * math.sqrt(max(layers, 1))
    assert gate_l2_fp8(layers) == 4e-2 + 4e-2 * math.sqrt(max(layers, 1))
    assert gate_l2(0) == gate_l2(1) and gate_l2_fp8(0) == gate_l2_fp8(1)


def test_metrics_on_known_tensors():
    a = torch.tensor([[3.0, 4.0], [1.0, 0.0]])
    b = torch.tensor([[3.0, 4.0], [0.0, 1.0]])
    assert rel_l2(a, a) == 0.0 and min_cos(a, a) == pytest.approx(1.0, abs=1e-15)
    assert rel_l2(a, b) == pytest.approx(math.sqrt(2.0 / 26.0), rel=1e-12)  # |a - b|^2 = 2, |b|^2 = 26
    assert min_cos(a, b) == pytest.approx(0.0, abs=1e-15)                   # the worst row decides
    assert min_cos(a.reshape(1, 2, 2), b.reshape(1, 2, 2)) == pytest.approx(0.0, abs=1e-15)  # rows are the last axis


def test_parity_passes_inside_the_gate(ref, capsys):
    check_parity(ref, ref, "equal", GATE)
    check_parity(ref * (1 + 0.9 * GATE), ref, "0.9 gate", GATE)
    check_parity(ref.to(torch.bfloat16), ref, "bf16 in, emulation given", GATE, ref_emul=ref.to(torch.bfloat16).float(), l2_emul=1e-9)
    check_parity(ref.reshape(8, ROWS // 8, COLS), ref.reshape(8, ROWS // 8, COLS), "3-D", GATE)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 4 and all(ln.count("gate") >= 2 for ln in out)  # one line per call, with the values and the gates
    assert "emulating" in out[2] and "emulating" not in out[0]


def test_parity_rejects_a_rel_l2_above_the_gate(ref):
    with pytest.raises(AssertionError, match="rel L2 vs fp32"):
        check_parity(ref * (1 + 1.1 * GATE), ref, "1.1 gate", GATE)


def test_parity_rejects_one_nan(ref):
    bad = ref.clone()
    bad[ROWS // 2, 3] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        check_parity(bad, ref, "nan", GATE)
    bad[ROWS // 2, 3] = float("inf")
    with pytest.raises(AssertionError, match="not finite"):
        check_parity(bad, ref, "inf", GATE)


def test_parity_rejects_one_rotated_row(ref):
    bad = _rotate_row(ref, 1234, 0.99)
    # one bad row among ROWS moves the overall rel L2 by sqrt(2 - 2 cos) / sqrt(ROWS) ~ 2.2e-3: the cosine check alone sees it
    assert rel_l2(bad, ref) <= 0.25 * GATE and min_cos(bad, ref) == pytest.approx(0.99, abs=1e-6)
    with pytest.raises(AssertionError, match="min cosine"):
        check_parity(bad, ref, "rotated row", GATE)
    check_parity(bad, ref, "rotated row, floor 0.98", GATE, cos=0.98)  # the floor is the caller's, as are the gates


def test_parity_rejects_the_emulating_reference_alone(ref):
    emul = ref * (1 + 2.2 * GATE)
    assert rel_l2(ref, emul) > GATE
    with pytest.raises(AssertionError, match="bf16-emulating"):
        check_parity(ref, ref, "emul off", GATE, ref_emul=emul)
    with pytest.raises(AssertionError, match="bf16-emulating"):
        check_parity(ref, ref, "emul off, own gate", 10 * GATE, ref_emul=emul, l2_emul=GATE)
    check_parity(ref, ref, "emul inside its own gate", GATE, ref_emul=emul, l2_emul=3 * GATE)


@pytest.mark.parametrize("what", ["one column", "one row", "flattened"])
def test_parity_rejects_another_shape_before_anything_broadcasts(ref, what):
    got = {"one column": ref[:, :1], "one row": ref[:1], "flattened": ref.reshape(-1)}[what]
    with pytest.raises(AssertionError, match="shape"):
        check_parity(got, ref, what, 1e9, cos=-1.0)  # (gates that nothing could miss: the shape check is what fires)


def test_fp8_gate_has_its_own_levels(ref):
    g8 = gate_l2_fp8(12)
    got = _rotate_row(ref, 77, 0.995) * (1 + 0.9 * g8)
    check_parity_fp8(got, ref, ref, 12, "fp8 inside")
    with pytest.raises(AssertionError, match="min cosine"):
        check_parity_fp8(_rotate_row(ref, 77, 0.985), ref, ref, 12, "fp8 row at 0.985")
    with pytest.raises(AssertionError, match="rel L2 vs fp32"):
        check_parity_fp8(ref * (1 + 1.1 * g8), ref, ref * (1 + 1.1 * g8), 12, "fp8 1.1 gate")
    with pytest.raises(AssertionError, match="MX-emulating"):
        check_parity_fp8(ref, ref, ref * (1 + 1.5 * g8), 12, "fp8 emul off")


def _batch(B=8):
    """small integers: every sum below is exact, so bitwise comparisons do not hinge on a summation order"""
    x = torch.randint(-8, 9, (B, 5), generator=torch.Generator().manual_seed(B)).float()
    x[B - 1] = x[1]
    return x


def test_batch_properties_pass_for_a_per_row_function():
    x = _batch()
    out = check_batch_properties(lambda t: t * t * 2 + 1, x)
    assert torch.equal(out, x * x * 2 + 1)
    check_batch_properties(lambda t: t.sum(1), _batch(6), small=1, perm=[3, 0, 5, 2, 4, 1], lo=2)


def test_batch_properties_reject_a_function_that_mixes_rows():
    # subtracting the batch mean keeps duplicates equal and commutes with a permutation: only the sub-batch run shows it
    with pytest.raises(AssertionError, match="depends on its batch"):
        check_batch_properties(lambda t: t - t.mean(0, keepdim=True), _batch())


def test_batch_properties_reject_a_function_of_the_position_in_the_batch():
    def by_position(t):
        pos = torch.arange(t.shape[0], dtype=t.dtype)
        return t + torch.minimum(pos, t.shape[0] - pos)[:, None]  # (equal at positions 1 and B - 1: duplicates still agree)
    with pytest.raises(AssertionError, match="permutation"):
        check_batch_properties(by_position, _batch())
    with pytest.raises(AssertionError, match="duplicate"):
        check_batch_properties(lambda t: t + torch.arange(t.shape[0], dtype=t.dtype)[:, None], _batch())
    with pytest.raises(AssertionError, match="not finite"):
        check_batch_properties(lambda t: t / 0, _batch())
