"""CPU: the attention checks of tests/test_attention_exact_gpu.py and the random-data beta gate bite.

oracle/attn_designs.py models the kernels' arithmetic (bf16 inputs, fp32 scores, RNE bf16 P, fp32 accumulation, bf16
output).  Without a bug the model passes every check; each injected bug is rejected by the checks named for it; and the
constructions have the properties the exactness argument rests on (gaps, zero-sum deviations, distinct c)."""
import math

import pytest
import torch

from oracle import attn_designs as ad

PAD_VALUES = (0.0, 1000.0, float("nan"), float("inf"), float("-inf"))
LENS = [1, 2, 15, 16, 17, 31, 33, 64, 65, 129, 160]  # padded to N = 160


def _model_on_packed(qkv, B, N, H, dh, lens, bug=None):
    q, k, v = ad.unpack_qkv(qkv, B, N, H, dh)
    return ad.model_attention(q, k, v, lens, bug=bug)


def _uniform(bug, B=2, N=197, H=3, dh=64):
    c = ad.uniform_case(B, N, H, dh, seed=1)
    ad.check_exact(ad.model_attention(c["q"], c["k"], c["v"], bug=bug), c["expected"], what="uniform")


def _onehot(bug, B=2, N=197, H=3, dh=64):
    c = ad.onehot_case(B, N, H, dh, seed=2)
    ad.check_exact(ad.model_attention(c["q"], c["k"], c["v"], bug=bug), c["expected"], what="one-hot")


def _random_beta(bug, B=2, N=197, H=3, dh=64):
    g = torch.Generator().manual_seed(3)
    q, k, v = (ad.bf16_round(torch.randn(B, N, H, dh, generator=g)) for _ in range(3))
    got = ad.model_attention(q, k, v, bug=bug)
    assert got.numel() >= ad.BETA_MIN_N
    ad.check_unbiased(got, ad.ref_attention(q, k, v), "random")


def _lengths(make, bug, N=160, H=2, dh=64):
    """padded sequences: valid rows exactly the construction's output, whatever the padding holds"""
    B = len(LENS)
    c = make(B, N, H, dh, lens=LENS, seed=4)
    rows = ad.valid_rows(c["lens"], N)
    qkv = ad.pack_qkv(c["q"], c["k"], c["v"])
    ad.check_exact(_model_on_packed(qkv, B, N, H, dh, c["lens"], bug), c["expected"], rows, "lengths")
    return c, qkv, rows


def _lengths_uniform(bug):
    _lengths(ad.uniform_case, bug)


def _lengths_onehot(bug):
    _lengths(ad.onehot_case, bug)


def _padding_contents(bug, N=160, H=2, dh=64):
    B = len(LENS)
    c, qkv, rows = _lengths(ad.uniform_case, None if bug == "nan_padding" else bug)
    for val in PAD_VALUES:
        got = _model_on_packed(ad.fill_padding(qkv, c["lens"], N, val), B, N, H, dh, c["lens"], bug)
        ad.check_exact(got, c["expected"], rows, f"padding {val}")


CHECKS = {"uniform": _uniform, "one-hot": _onehot, "beta": _random_beta, "lengths-uniform": _lengths_uniform,
          "lengths-one-hot": _lengths_onehot, "padding-contents": _padding_contents}

# which checks must reject which bug (the others may or may not)
REJECTED_BY = {
    "drop_key": ("uniform", "one-hot"),
    "extra_zero_key": ("uniform", "beta"),
    "dup_last_key": ("uniform",),  # (beta: by how much depends on the last key's V)
    "trunc_p": ("beta",),
    "temperature": ("beta",),
    "cross_head_k": ("one-hot", "beta"),
    "len_off_by_one": ("lengths-uniform", "lengths-one-hot"),
    "nan_padding": ("padding-contents",),
}


@pytest.mark.parametrize("check", sorted(CHECKS))
def test_every_check_passes_the_bug_free_model(check):
    CHECKS[check](None)


@pytest.mark.parametrize("bug", ad.BUGS)
def test_each_injected_bug_is_rejected(bug):
    assert set(REJECTED_BY) == set(ad.BUGS)
    for check in REJECTED_BY[bug]:
        with pytest.raises(AssertionError):
            CHECKS[check](bug)


def test_beta_of_a_correct_model_is_far_below_the_gate_and_the_bugs_far_above():
    """the margins the gate rests on: ~1e-5 for RNE rounding, >= 1e-3 for the P rounding, temperature and denominator
    bugs, which move every output the same way"""
    g = torch.Generator().manual_seed(5)
    B, N, H, dh = 2, 197, 3, 64
    q, k, v = (ad.bf16_round(torch.randn(B, N, H, dh, generator=g)) for _ in range(3))
    ref = ad.ref_attention(q, k, v)
    assert abs(ad.beta(ad.model_attention(q, k, v), ref)) < 3e-5
    for bug in ("trunc_p", "temperature", "extra_zero_key"):
        assert abs(ad.beta(ad.model_attention(q, k, v, bug=bug), ref)) > 1e-3, bug
    assert ad.check_unbiased(torch.zeros(100), torch.ones(100)) is None  # below BETA_MIN_N: no gate


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 16, 17, 64, 65, 197, 1024])
def test_zero_sum_deviations(L):
    g = torch.Generator().manual_seed(L)
    d = ad.zero_sum_deviations(L, g)
    assert d.shape == (L,) and d.sum() == 0 and d.abs().max() <= 14
    assert L == 1 or (d != 0).all()


@pytest.mark.parametrize("B,N,H,dh", [(171, 197, 3, 64), (2, 1024, 3, 128), (4, 65, 2, 32), (3, 129, 2, 96)])
def test_uniform_construction_properties(B, N, H, dh):
    lens = torch.randint(1, N + 1, (B,), generator=torch.Generator().manual_seed(N))
    lens[0] = N
    c = ad.uniform_case(B, N, H, dh, lens=lens, seed=6)
    assert (c["q"] == 0).all()
    assert torch.equal(ad.bf16_round(c["v"]), c["v"]) and torch.equal(ad.bf16_round(c["k"]), c["k"])
    assert (c["c"][..., 0::2] == 0).all()
    odd = c["c"][..., 1::2].reshape(-1)
    assert odd.unique().numel() == odd.numel(), "c is not distinct per (b, h, col)"
    for b in range(B):
        L = int(lens[b])
        d = c["d"][b, :, :L]
        assert (d.sum(-1) == 0).all()
        assert L == 1 or (d != 0).all()
        # valid V rows: whole numbers of the (b, h) pair's power-of-two unit, below 256 of them (so every partial sum
        # of up to 2^16 keys is exact in fp32)
        units = c["v"][b, :L] / c["unit"][b][None, :, None]
        assert torch.equal(units, units.round()) and (units.abs() < 256).all()
    assert torch.equal(c["expected"][:, 0], c["c"])


@pytest.mark.parametrize("B,N,H,dh,lens", [(2, 197, 3, 64, None), (3, 289, 2, 32, [289, 17, 1]), (2, 1024, 1, 128, None),
                                           (2, 129, 2, 96, [128, 65])])
def test_onehot_construction_properties(B, N, H, dh, lens):
    c = ad.onehot_case(B, N, H, dh, lens=lens, seed=7)
    assert c["gap_nats"] >= ad.GAP_NATS
    lens = c["lens"]
    a = c["a"]
    assert a == 2.0 ** round(math.log2(a))
    for b in range(B):
        L = int(lens[b])
        for h in range(H):
            k, q, v = c["k"][b, :, h], c["q"][b, :, h], c["v"][b, :, h]
            s = (q[:L] @ k[:L].t()) / math.sqrt(dh)
            top2 = s.topk(min(2, L), dim=-1).values
            target = s.argmax(-1)
            assert torch.equal(v[target], c["expected"][b, :L, h])
            assert sorted(target.tolist()) == list(range(L)), "pi is not a permutation of the valid keys"
            if L > 1:
                assert (top2[:, 0] - top2[:, 1]).min() >= ad.GAP_NATS
            # adversarial padding: a leaked padding key outscores the target
            if L < N:
                assert ((q[:L] @ k[L:].t()).max(-1).values > s.max(-1).values * math.sqrt(dh)).any()
    assert ((c["v"].abs() >= 1) & (c["v"].abs() < 2))[ad.valid_rows(lens, N)].all()


@pytest.mark.parametrize("delta", [(0, 0), (1, -2), (-3, 1)])
def test_relpos_spike_construction(delta):
    from oracle import sam_oracle as so
    S = 7
    c = ad.relpos_spike_case(1, S, 1, delta)
    q = c["q"][0, :, 0]
    Rh, Rw = so.rel_table(S, c["rel_h"]), so.rel_table(S, c["rel_w"])
    bias = torch.einsum("hwc,hkc->hwk", q.reshape(S, S, 64), Rh)[..., :, None] + \
        torch.einsum("hwc,wkc->hwk", q.reshape(S, S, 64), Rw)[..., None, :]
    bias = bias.reshape(S * S, S * S)
    t = c["target"]
    inside = t >= 0
    assert inside.any() and ((~inside).any() or delta == (0, 0))
    assert torch.equal(bias[inside].argmax(-1), t[inside])
    top2 = bias[inside].topk(2, dim=-1).values
    assert (top2[:, 0] - top2[:, 1]).min() >= ad.GAP_NATS
