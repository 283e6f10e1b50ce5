"""CPU: the tools of the memory-contract and core-operator edge tests check themselves -- memguard detects what it claims
to detect, the designed inputs of tests/core_ops_designs.py give their integers under an fp32 restatement of the device
formulas and lose them under every planted bug, and the derived LayerNorm bound admits a two-pass fp32 kernel and
rejects a one-pass one."""
import pytest
import torch

import core_ops_designs as cd
import memguard as mg

SWIGLU_SHAPES = [(1, 64, 64), (7, 128, 64), (129, 320, 128), (257, 576, 192)]


# ---- memguard ---------------------------------------------------------------------------------------------------------
def test_memguard_detects_one_byte_before_and_after_the_body():
    guard, n = 512, 1000
    whole, body = mg.guarded(n, guard, device="cpu")
    assert body.numel() == n and mg.guards_intact(whole, guard)
    body.fill_(0)  # the body itself is the callee's to write
    assert mg.guards_intact(whole, guard)
    for off in (-1, -guard, n, n + guard - 1):  # nearest and farthest guard byte on either side
        w, b = mg.guarded(n, guard, device="cpu")
        w[guard + off] = mg.CANARY ^ 1
        assert not mg.guards_intact(w, guard), off
        front, back = mg.guard_damage(w, guard)
        assert (front if off < 0 else back) == off


def test_memguard_row_helpers():
    whole, body = mg.guarded_rows(5, 8, torch.bfloat16, guard_rows=2, device="cpu")
    assert body.shape == (5, 8) and mg.rows_intact(whole, 2) and mg.canary_left(body) == 40
    body.copy_(torch.ones(5, 8))
    assert mg.canary_left(body) == 0 and mg.rows_intact(whole, 2)
    body[3, 4] = mg.canary_value(torch.bfloat16)
    assert mg.canary_left(body) == 1
    whole[1, 7] = 0.0
    assert not mg.rows_intact(whole, 2)
    whole, body = mg.guarded_rows(5, 8, torch.float32, guard_rows=2, device="cpu")
    whole[7, 0] = 0.0
    assert not mg.rows_intact(whole, 2)
    t = torch.arange(12.0).view(3, 4)
    v = mg.inside_nan(t, pad=4, device="cpu")
    assert torch.equal(v, t) and v.is_contiguous()
    big = v.untyped_storage()
    assert big.nbytes() == (3 + 8) * 4 * 4


def _decode(raw: torch.Tensor, kind: str) -> torch.Tensor:
    """bytes -> values as float64 under one of the four element types a workspace holds"""
    if kind == "bf16":
        return raw.view(torch.bfloat16).double()
    if kind == "fp32":
        return raw.view(torch.float32).double()
    if kind == "e4m3":
        return raw.view(torch.float8_e4m3fn).double()
    # e8m0 (OCP MX block scale): 2^(byte - 127), 0xFF = NaN
    b = raw.double()
    return torch.where(raw == 255, torch.full_like(b, float("nan")), torch.exp2(b - 127.0))


@pytest.mark.parametrize("name", sorted(mg.FILLS))
def test_fill_patterns_are_what_they_claim(name):
    whole, body = mg.guarded(4096, 256, device="cpu")
    mg.fill(body, name)
    assert mg.guards_intact(whole, 256)
    for kind, what in mg.FILL_MEANS[name].items():
        v = _decode(body.clone(), kind)
        if what == "nan":
            assert torch.isnan(v).all(), (name, kind)
        elif what == "1000":
            assert (v == 1000.0).all(), (name, kind)
        elif what == "zero":
            assert (v == 0.0).all(), (name, kind)
        else:
            assert (v > 0).all() and (v < 1e-37).all(), (name, kind)
    # a partial fill continues the whole pattern
    w2, b2 = mg.guarded(4096, 256, device="cpu")
    mg.fill(b2, name, 0, 1024)
    mg.fill(b2, name, 1024, 4096)
    assert torch.equal(b2, body)
    assert set(mg.FILL_MEANS["ones"]) == {"bf16", "fp32", "e4m3", "e8m0"}


# ---- SwiGLU design ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", SWIGLU_SHAPES)
def test_swiglu_design_gives_its_integers_exactly(M, N, K):
    x, W, b, bit = cd.swiglu_design(M, N, K)
    for t in (x, W, b):
        assert torch.equal(t, t.to(torch.bfloat16).float()) and torch.equal(t, t.round())
    pre = x @ W.t() + b
    gate = pre.view(M, N // 64, 2, 32)[:, :, 0].reshape(M, N // 2)
    assert torch.equal(gate, torch.where(bit, 32.0, -128.0))
    want = cd.swiglu_expected(x, W, b, bit)
    assert want.abs().max() <= 224 and torch.equal(want, want.round())
    got = cd.swiglu_eval(x, W, b)
    assert torch.equal(got.float(), want)  # (+0 == -0: the sign of a zero is the restatement's, compared on the GPU)
    assert bool(bit.any()) and (M == 1 or bool((~bit).any()))
    assert (want != 0).sum() > 0.2 * bit.sum()


def test_silu_saturates_as_the_design_says():
    assert cd.silu_f32(torch.tensor([32.0])).item() == 32.0
    z = cd.silu_f32(torch.tensor([-128.0]))
    assert z.item() == 0.0 and torch.signbit(z).item()
    assert float(torch.exp2(torch.tensor(-32.0 * cd.LOG2E))) < 2.0 ** -25


@pytest.mark.parametrize("bug", cd.SWIGLU_BUGS)
@pytest.mark.parametrize("M,N,K", SWIGLU_SHAPES)
def test_swiglu_design_notices_every_planted_bug(M, N, K, bug):
    x, W, b, bit = cd.swiglu_design(M, N, K)
    good = cd.swiglu_eval(x, W, b)
    bad = cd.swiglu_eval(x, W, b, bug=bug)
    if bug == "plain_column" and N == 64:  # one block of 64: the permuted and the plain output column coincide
        assert torch.equal(good.view(torch.int16), bad.view(torch.int16))
        return
    assert not torch.equal(good.view(torch.int16), bad.view(torch.int16)), bug


# ---- saturated GELU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(cd.GELU_FORMS))
def test_gelu_forms_return_the_integer_after_bf16_rounding(form):
    lo, hi = cd.GELU_RANGE
    v = torch.arange(lo, hi + 1).float()
    y = cd.GELU_FORMS[form](v)
    assert torch.equal(y.to(torch.bfloat16).float(), v), form
    # the margin: the fp32 value is within 2^-12 relative of the integer, against the 2^-9 of a bf16 half ulp, so 1-ulp
    # differences of the device's exp2 / rcp cannot move the rounded result
    assert ((y - v).abs() <= v * 2.0 ** -12).all()
    # ... and the design is not vacuous: below the range the forms do not return their argument
    assert cd.GELU_FORMS[form](torch.tensor([1.0])).to(torch.bfloat16).item() != 1.0


@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (7, 72, 64), (65, 136, 128), (129, 264, 192), (257, 520, 64)])
def test_gelu_design_codes_rows_and_columns(M, N, K):
    x, W, b, want = cd.gelu_design(M, N, K)
    for t in (x, W, b):
        assert torch.equal(t, t.to(torch.bfloat16).float())
    assert torch.equal(x @ W.t() + b, want)
    assert N < 2 or not torch.equal(want[:, 0], want[:, 1])
    assert M < 2 or not torch.equal(want[0], want[1])


# ---- LayerNorm bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dt,out_dt", [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
                                          (torch.float32, torch.bfloat16), (torch.float32, torch.float32)])
def test_ln_bound_holds_for_a_two_pass_fp32_kernel(in_dt, out_dt):
    worst = 0.0
    for D in cd.LN_WIDTHS:
        for rows in cd.LN_ROWS:
            x, g, b = cd.ln_inputs(D, rows, in_dt)
            for eps in (1e-6, 1e-5):
                r = cd.worst_ratio(cd.ln_two_pass_fp32(x, g, b, eps, out_dt), x, g, b, eps, out_dt)
                assert r <= 1.0, (D, rows, eps, r)
                worst = max(worst, r)
    print(f"two-pass emulation {in_dt} -> {out_dt}: worst error / bound {worst:.3f}")
    assert worst > 0.01  # the bound is not so loose that it could not notice anything


def test_ln_offset_case_separates_two_pass_from_one_pass():
    x, g, b = cd.ln_offset_case()
    eps = 1e-6
    two = cd.worst_ratio(cd.ln_two_pass_fp32(x, g, b, eps, torch.float32), x, g, b, eps, torch.float32)
    one = cd.worst_ratio(cd.ln_one_pass_fp32(x, g, b, eps, torch.float32), x, g, b, eps, torch.float32)
    print(f"offset case: two-pass ratio {two:.3f}, one-pass ratio {one:.1f}")
    assert two <= 1.0
    assert one > 1.0
    # also with a bf16 store: the rounding of the output does not hide a broken variance
    one_bf = cd.worst_ratio(cd.ln_one_pass_fp32(x, g, b, eps, torch.bfloat16), x, g, b, eps, torch.bfloat16)
    assert one_bf > 1.0


def test_ln_bound_is_tighter_than_the_old_flat_tolerance_where_it_matters():
    """At the widths the old test used (|y| of order 1) the fp32-output bound is far below 2e-5 + 2e-5 |ref|."""
    x, g, b = cd.ln_inputs(768, 9, torch.float32)
    bound = cd.ln_bound(x, g, b, 1e-6, torch.float32)
    flat = 2e-5 + 2e-5 * cd.ln_ref64(x, g, b, 1e-6).abs()
    assert (bound < flat / 4).all()
