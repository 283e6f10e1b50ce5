"""GPU: every attention kernel on designed inputs whose bf16 output is known exactly, compared bit for bit.

The constructions (oracle/attn_designs.py; tests/test_attention_gates_cpu.py shows on a model of the kernels' arithmetic
that each rejects the bugs it is meant to catch):
  uniform   Q = 0 so P = 1; V = c + zero-sum integer deviations: every valid row is exactly c -- a dropped, extra or
            duplicated key, or a row routed from another (sequence, head, column), changes bits
  one-hot   Q_i = a K_pi(i) for +-1 codes with a >= 24-nat gap: row i is exactly V[pi(i)] -- pins the key permutation,
            the head routing and, where pi crosses key chunks, the online-softmax rescale
  relpos    the same with zero rel-pos tables, and a spike in each table that makes the bias alone pick one key
  lengths   padded sequences through vdr_op_attention_varlen: exact on the valid rows, bitwise independent of what the
            padding rows hold (0, 1000, NaN, +-Inf) and bitwise equal to the sequence run alone, unpadded

Code paths (csrc/attention.hip launch_attention): at head dim 64, variant 3 is the one-shot kernel (NT 2 / 4 / 7 / 9 by
length), 1 the online softmax (and every length > 288), 2 the persistent kernel without its loader wave (<4,false> up
to 128 tokens, <7,false> to 224), 4 the one with it (<7,true>, 129..224 tokens), 0 the library's choice (<7,true> from
512 (sequence, head) items on).  Head dims 32 / 96 / 128 run one kernel (attention_hd.hip) whatever the variant."""
import pytest
import torch

from fixtures import ops  # noqa: F401
from oracle import attn_designs as ad

pytestmark = pytest.mark.gpu

N64 = [1, 5, 32, 33, 64, 65, 128, 129, 197, 224, 225, 288, 289, 577, 1024]
NHD = [1, 5, 32, 33, 63, 64, 65, 127, 128, 129, 197, 224, 225, 288, 289, 577, 1024]  # + key-chunk edges KC +- 1
PAD_VALUES = (0.0, 1000.0, float("nan"), float("inf"), float("-inf"))
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 224, 225, 288, 289, 513]


def _variants(dh):
    return (0, 1, 2, 3, 4) if dh == 64 else (0, 1)


def _run(ops, qkv, B, N, H, dh, variant, lengths=None, len_add=0):
    o = ops.attention(qkv, B, N, H, variant=variant, head_dim=dh, lengths=lengths, len_add=len_add)
    return o.reshape(B, N, H, dh)


def _exact_all_variants(ops, case, B, N, H, dh, what, variants=None):
    qkv = ad.pack_qkv(case["q"], case["k"], case["v"]).cuda()
    for v in variants or _variants(dh):
        ad.check_exact(_run(ops, qkv, B, N, H, dh, v), case["expected"], what=f"{what} variant {v}")


# ---- fixed length -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,N", [(64, n) for n in N64] + [(dh, n) for dh in (32, 96, 128) for n in NHD])
def test_uniform_attention_is_exact(ops, dh, N):
    B, H = 2, 3
    c = ad.uniform_case(B, N, H, dh, seed=N + dh)
    _exact_all_variants(ops, c, B, N, H, dh, f"uniform dh{dh} N{N}")


@pytest.mark.parametrize("dh,N", [(64, n) for n in N64] + [(dh, n) for dh in (32, 96, 128) for n in NHD])
def test_onehot_permutation_is_exact(ops, dh, N):
    B, H = 2, 3
    c = ad.onehot_case(B, N, H, dh, seed=7 * N + dh, device="cuda")
    assert c["gap_nats"] >= ad.GAP_NATS
    _exact_all_variants(ops, c, B, N, H, dh, f"one-hot dh{dh} N{N}")


@pytest.mark.parametrize("N", [129, 197, 224])
def test_persistent_kernels_are_exact_from_512_items(ops, N):
    """171 x 3 = 513 (sequence, head) items: variant 0 runs persist<7,true>, 2 persist<7,false>, 4 persist<7,true>"""
    B, H = 171, 3
    _exact_all_variants(ops, ad.uniform_case(B, N, H, 64, seed=N), B, N, H, 64, f"uniform 513 items N{N}", (0, 2, 3, 4))
    c = ad.onehot_case(B, N, H, 64, seed=N + 1, device="cuda")
    _exact_all_variants(ops, c, B, N, H, 64, f"one-hot 513 items N{N}", (0, 2, 3, 4))


# ---- SAM relative position bias ---------------------------------------------------------------------------------
def _relpos(ops, c, B, S, H):
    qkv = ad.pack_qkv(c["q"], c["k"], c["v"]).cuda()
    return ops.attention_relpos(qkv, c["rel_h"].cuda(), c["rel_w"].cuda(), B, S, H).reshape(B, S * S, H, 64)


@pytest.mark.parametrize("B,S,H", [(3, 4, 2), (5, 7, 1), (2, 10, 2), (4, 14, 3), (1, 64, 2)])
def test_relpos_onehot_with_zero_tables_is_exact(ops, B, S, H):
    c = ad.relpos_onehot_case(B, S, H, seed=S, device="cuda")
    assert c["gap_nats"] >= ad.GAP_NATS
    ad.check_exact(_relpos(ops, c, B, S, H), c["expected"], what=f"relpos one-hot S{S}")


@pytest.mark.parametrize("S", [4, 7, 10, 14, 64])
@pytest.mark.parametrize("delta", [(0, 0), (1, -2), (-3, 1)])
def test_relpos_bias_picks_the_key_it_points_at(ops, S, delta):
    """The bias alone selects key (qh - dh, qw - dw): exact where that key is in the grid (pins the qh - kh direction
    and the table packing); the other queries (ties of several keys) against float64."""
    from oracle import sam_oracle as so
    B, H = 2, 2
    c = ad.relpos_spike_case(B, S, H, delta, seed=S)
    got = _relpos(ops, c, B, S, H)
    t = c["target"]
    inside = t >= 0
    want = c["v"][:, t.clamp(min=0)]
    ad.check_exact(got[:, inside], want[:, inside], what=f"relpos spike S{S} delta{delta}")
    if (~inside).any():
        n = S * S
        q, k, v = (x.cuda().double().permute(0, 2, 1, 3) for x in (c["q"], c["k"], c["v"]))
        Rh = so.rel_table(S, c["rel_h"].double()).cuda()
        Rw = so.rel_table(S, c["rel_w"].double()).cuda()
        rq = q.reshape(B, H, S, S, 64)
        bias = torch.einsum("bnhwc,hkc->bnhwk", rq, Rh)[..., :, None] + torch.einsum("bnhwc,wkc->bnhwk", rq, Rw)[..., None, :]
        s = (q @ k.transpose(-1, -2)) / 8 + bias.reshape(B, H, n, n)
        ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).float().cpu()
        g, r = got[:, ~inside].float().cpu(), ref[:, ~inside]
        assert ((g - r).abs() <= 6e-3 + 2 * 2.0 ** -8 * r.abs()).all(), f"relpos spike S{S}: max err {(g - r).abs().max():.3g}"


# ---- per-sequence lengths -------------------------------------------------------------------------------------------
def _random_case(B, N, H, dh, lens, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (ad.bf16_round(torch.randn(B, N, H, dh, generator=g)) for _ in range(3))
    return dict(q=q, k=k, v=v, expected=None, lens=ad.check_lens(B, N, lens))


MAKERS = {"uniform": lambda *a, **kw: ad.uniform_case(*a, **kw),
          "one-hot": lambda *a, **kw: ad.onehot_case(*a, device="cuda", **kw),
          "random": _random_case}


@pytest.mark.parametrize("dh,seq", [(64, 64), (64, 128), (64, 224), (64, 288), (64, 600),
                                    (32, 129), (32, 600), (96, 65), (96, 600), (128, 65), (128, 600)])
@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_lengths_are_exact_and_padding_does_not_leak(ops, dh, seq, kind):
    """One batch holds every length of LENGTHS that fits (plus one whose lens[b] + len_add exceeds seq: clipped),
    run with len_add 0 and 1 through vdr_op_attention_varlen.  Valid rows: exact (uniform, one-hot) or within bf16 of
    float64 (random); bitwise the same whatever the padding rows hold; bitwise equal to the sequence run alone, unpadded,
    with the same variant (at dh 64 variant 1, the online kernel both times: otherwise a batch padded past 288 tokens
    runs the online kernel and a lone sequence of up to 288 the one-shot kernel, whose sums are ordered differently)."""
    H = 2
    eff = [n for n in LENGTHS if n <= seq] + [seq]
    B = len(eff)
    case = MAKERS[kind](B, seq, H, dh, lens=eff, seed=seq + dh)
    lens = case["lens"]
    rows = ad.valid_rows(lens, seq)
    base = ad.pack_qkv(case["q"], case["k"], case["v"]).cuda()
    if case["expected"] is None:
        ref = ad.ref_attention(case["q"], case["k"], case["v"], lens, device="cuda").float().cpu()
    for len_add in (0, 1):
        arg = lens - len_add
        arg[-1] = seq + 3 - len_add  # past the padded length: clipped to seq
        for variant in _variants(dh):
            what = f"{kind} dh{dh} seq{seq} len_add{len_add} variant{variant}"
            got = _run(ops, base, B, seq, H, dh, variant, arg, len_add)
            if case["expected"] is not None:
                ad.check_exact(got, case["expected"], rows, what)
            else:
                g, r = got.float().cpu()[rows], ref[rows]
                assert ((g - r).abs() <= 6e-3 + 2 * 2.0 ** -8 * r.abs()).all(), f"{what}: max err {(g - r).abs().max():.3g}"
            for val in PAD_VALUES:
                other = _run(ops, ad.fill_padding(base, lens, seq, val), B, seq, H, dh, variant, arg, len_add)
                ad.check_exact(other, got, rows, f"{what} padding {val}")
        ref_variant = 1 if dh == 64 else 0
        padded = _run(ops, base, B, seq, H, dh, ref_variant, arg, len_add)
        for b, L in enumerate(lens.tolist()):
            alone = _run(ops, base[b * seq:b * seq + L].contiguous(), 1, L, H, dh, ref_variant)
            ad.check_exact(padded[b, :L], alone[0], what=f"{kind} dh{dh} seq{seq} len {L} alone vs padded")
