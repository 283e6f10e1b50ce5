"""CPU: the checks of tests/test_ln_fold_gpu.py bite, and the exported host fold is the float64 arithmetic.

oracle/ln_fold_designs.py models the fold (fp32 partials per 64 columns of the stored bf16 rows, double finalisation,
fp32 epilogue, bf16 RNE store).  Without a bug the model passes every check; each injected bug is rejected by the check
named for it."""
import pytest
import torch

from oracle import ln_fold_designs as lf

M, D, N = 40, 768, 128


@pytest.fixture(scope="module")
def case():
    x = lf.cycled_rows(M, D, seed=3)
    W, b, gamma, beta = lf.designed_weights(N, D, seed=4)
    Wf, cs, tb = lf.model_fold(W, b, gamma, beta)
    return x, W, b, gamma, beta, Wf, cs, tb, lf.ref_fold(x, Wf, W, b, beta), lf.fold_noise_scale(x, Wf, cs, tb)


def _consumer_check(case, stats_bug=None, fold_bug=None):
    x, W, b, gamma, beta, Wf, cs, tb, ref, scale = case
    if fold_bug:
        Wf, cs, tb = lf.model_fold(W, b, gamma, beta, bug=fold_bug)
    st = lf.model_finalize(lf.model_partials(x), bug=stats_bug)
    return lf.check_exact_bf16(lf.model_consumer(x, Wf, cs, tb, st), ref, f"{stats_bug or fold_bug}", scale=scale,
                               max_excluded_frac=0.1)


def test_designed_rows_have_the_stated_moments():
    x = lf.cycled_rows(30, D, seed=1)
    for r in range(30):
        mu, sigma = lf.ROW_CLASSES[r % len(lf.ROW_CLASSES)]
        assert x[r].double().mean().item() == mu
        v = x[r].double().var(unbiased=False).item()
        assert v == pytest.approx(sigma ** 2 * (0.5 if r % 2 == 0 else 2 / 3), rel=1e-12)
    assert {abs(m) / s for m, s in lf.ROW_CLASSES if s > 0} >= {0.0, 16.0, 64.0, 192.0}


def test_bug_free_model_passes_the_exact_checks(case):
    n = _consumer_check(case)
    assert n <= 0.1 * M * N, n


@pytest.mark.parametrize("bug", ["unbiased", "eps_outside", "float_inv_d", "drop_last", "double_last", "neighbour"])
def test_each_statistics_bug_is_rejected(case, bug):
    with pytest.raises(AssertionError):
        _consumer_check(case, stats_bug=bug)


@pytest.mark.parametrize("bug", ["colsum_unrounded", "tbias_no_beta"])
def test_each_host_fold_bug_is_rejected(case, bug):
    with pytest.raises(AssertionError):
        _consumer_check(case, fold_bug=bug)


def test_float_inv_d_is_caught_by_the_large_mean_rows_only():
    """the shipped float 1/D moves nothing on rows with mean 0 and everything it moves sits on |mean| >> sigma"""
    W, b, gamma, beta = lf.designed_weights(N, D, seed=4)
    Wf, cs, tb = lf.model_fold(W, b, gamma, beta)
    for classes, caught in ((((0.0, 1.0), (0.0, 4.0)), False), ((((192.0, 1.0), (-192.0, 1.0)), True))):
        x = lf.cycled_rows(M, D, seed=5, classes=classes)
        ref, scale = lf.ref_fold(x, Wf, W, b, beta), lf.fold_noise_scale(x, Wf, cs, tb)
        got = lf.model_consumer(x, Wf, cs, tb, lf.model_finalize(lf.model_partials(x), bug="float_inv_d"))
        if caught:
            with pytest.raises(AssertionError, match="differ"):
                lf.check_exact_bf16(got, ref, scale=scale, max_excluded_frac=0.2)
        else:
            lf.check_exact_bf16(got, ref, scale=scale, max_excluded_frac=0.2)


def test_finaliser_model_is_the_float64_formula():
    g = torch.Generator().manual_seed(0)
    y = lf.bf16_round(torch.randn(50, D, generator=g) + 100)
    st = lf.model_finalize(lf.model_partials(y))
    yd = y.double()
    mean = yd.mean(1)
    rstd = 1 / torch.sqrt(yd.var(1, unbiased=False) + float(torch.tensor(lf.EPS, dtype=torch.float32)))
    assert torch.allclose(st[:, 0].double(), mean, rtol=1e-7, atol=0)
    assert torch.allclose(st[:, 1].double(), rstd, rtol=1e-6, atol=0)


def test_partials_check_rejects_statistics_of_the_pre_rounding_values():
    g = torch.Generator().manual_seed(1)
    y = torch.randn(64, D, generator=g) * 3
    yb = lf.bf16_round(y)
    lf.check_partials_of(lf.model_partials(y), yb, "stored rows")
    with pytest.raises(AssertionError):
        lf.check_partials_of(lf.model_partials(y, bug="prerounding"), yb, "pre-rounding")


def test_swiglu_colsum_bug_is_rejected():
    x = lf.cycled_rows(M, D, seed=6)
    W, b, gamma, beta = lf.designed_weights(256, D, seed=7)
    Wf, cs, tb = lf.model_fold(W, b, gamma, beta, swiglu=True)
    P = lf.swiglu_perm(256)
    lin = lf.ref_fold(x, Wf, W[P], b[P], beta).view(M, -1, 2, 32)
    ref = (torch.nn.functional.silu(lin[:, :, 0]) * lin[:, :, 1]).reshape(M, -1)
    st = lf.model_finalize(lf.model_partials(x))
    lf.check_close(lf.model_consumer(x, Wf, cs, tb, st, "swiglu"), ref, 2.0 ** -8, 2e-3, "swiglu")
    with pytest.raises(AssertionError):
        lf.check_close(lf.model_consumer(x, Wf, cs, tb, st, "swiglu", bug="swiglu_x1_colsum"), ref, 2.0 ** -8, 2e-3)


@pytest.mark.parametrize("swiglu", [False, True])
def test_exported_host_fold_against_float64(swiglu):
    from vdr import ops
    g = torch.Generator().manual_seed(11 + swiglu)
    Nn, K = 256, 192
    W = torch.randn(Nn, K, generator=g) * 0.05
    b = torch.randn(Nn, generator=g)
    gamma = 1 + 0.3 * torch.randn(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g)
    Wf, cs, tb = ops.ln_fold_weights(W, b, gamma, beta, swiglu=swiglu)
    if swiglu:
        Wp, bp = ops.pack_w12(W, b)
        assert torch.equal(Wp, W[lf.swiglu_perm(Nn)]) and torch.equal(bp, b[lf.swiglu_perm(Nn)])
        W, b = Wp, bp
    assert torch.equal(Wf.float(), (gamma * W).to(torch.bfloat16).float())  # bitwise bf16(gamma W)
    assert torch.equal(cs, Wf.double().sum(1).float())  # colsum of the ROUNDED weight, exactly
    want = (beta.double() @ W.double().t()) + b.double()
    ulp = torch.abs(torch.nextafter(want.float(), torch.tensor(float("inf"))) - want.float()).double()
    assert ((tb.double() - want).abs() <= ulp).all()  # within one fp32 ulp
