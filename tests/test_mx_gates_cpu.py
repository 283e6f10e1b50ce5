"""CPU: the checks of tests/test_mx_exact_gpu.py bite, and the designs are what they say.

oracle/mx_designs.py models the MX-fp8 path (the quantiser, LayerNorm to MX, the block-scaled GEMM's scale routing, the
re-quantising epilogue).  Without a bug the model passes every check; each injected bug is rejected, by name, by the
check that is meant to catch it."""
import os

import numpy as np
import pytest
import torch

from oracle import mx_designs as md
from oracle import mx_oracle as mx
from oracle.ln_fold_designs import bf16_round, swiglu_perm

LN_DIMS = (32, 96, 512, 544, 1536, 2048)
LN_ROWS = (1, 5, 130)


# ---- the raw encoding ---------------------------------------------------------------------------------------------
def test_raw_encoder_agrees_with_the_golden_table_for_all_256_bytes(golden_dir):
    g = np.load(os.path.join(golden_dir, "e4m3fn_table.npz"))
    tab = torch.from_numpy(g["decode"])
    assert np.array_equal(mx.e4m3_decode_table(), g["decode"], equal_nan=True)
    want = torch.arange(256, dtype=torch.uint8)
    for mode in ("rne", "trunc", "ties_away"):  # a value on the grid is its own rounding in every mode
        got = md.e4m3_round(tab, mode)
        fin = ~torch.isnan(tab)
        assert torch.equal(got[fin], want[fin]), mode
        assert bool(((got[~fin] & 0x7F) == 0x7F).all())
    # a block whose maximum is 448 has scale 2^0: the encoder returns the bytes themselves (block 0: the positive codes
    # 0x00 .. 0x7e in blocks of 32 each padded with 448; NaN codes left out)
    fin_codes = want[~torch.isnan(tab)]
    vals = tab[fin_codes.long()].reshape(-1, 1)
    x = torch.cat([vals, torch.full((vals.shape[0], 31), 448.0)], 1)
    q, s = md.encode(x)
    assert torch.equal(q[:, 0], fin_codes) and bool((s == 127).all())
    # and the golden quantiser vectors
    q, s = md.encode(torch.from_numpy(g["x"]))
    assert np.array_equal(q.numpy(), g["payload"]) and np.array_equal(s.numpy().astype(np.int32) - 127, g["exponent"])


def test_rounding_model_is_torchs_cast():
    g = torch.Generator().manual_seed(0)
    y = torch.cat([(torch.rand(20000, generator=g) * 2 - 1) * 448, (torch.rand(20000, generator=g) * 2 - 1) * 2.0 ** -5,
                   torch.arange(-1024, 1025) * 2.0 ** -11, torch.arange(-896, 897) * 0.5])
    assert torch.equal(md.e4m3_round(y), y.to(torch.float8_e4m3fn).view(torch.uint8))


def test_scale_exponent_is_the_exact_ceiling_for_every_bf16_maximum():
    """the kernels form amax * fl(1 / 448) in fp32; for every finite bf16 value that gives ceil(log2(amax / 448))"""
    allb = torch.arange(0, 0x7F80, dtype=torch.int16).view(torch.bfloat16).float()
    assert torch.equal(md.exact_scale_exponent(allb), mx.scale_exponent(allb))
    for k in (-126, -20, 0, 40, 118):
        e = md.exact_scale_exponent(torch.tensor([446.0, 448.0, 450.0]) * 2.0 ** k).tolist()
        assert e == [k, k, k + 1]
    assert md.exact_scale_exponent(torch.tensor([448.0 * 2.0 ** -127, 2.0 ** -133, 0.0])).tolist() == [-126] * 3


def test_scale_offsets_are_a_bijection_onto_the_padded_planes():
    for rows, K in ((1, 32), (65, 96), (300, 544), (513, 64)):
        off = md.mx_scale_offsets(rows, torch.arange(rows), K).reshape(-1)
        assert off.unique().numel() == rows * (K // 32) and int(off.max()) < md.mx_rows_pad(rows) * (K // 32)
        sb = torch.randint(0, 256, (rows, K // 32), dtype=torch.uint8)
        flat = md.place_scales(sb, fill=0x5A)
        assert torch.equal(md.gather_scales(flat, rows, K), sb)
        assert bool((flat[md.unwritten_mask(rows, K)] == 0x5A).all())
        assert int(md.unwritten_mask(rows, K).sum()) == (md.mx_rows_pad(rows) - rows) * (K // 32)
    # rows 0 and 32 are neighbours, row 64 starts the next group
    assert md.mx_scale_slot(torch.tensor([0, 32, 1, 33, 31, 63, 64])).tolist() == [0, 1, 2, 3, 62, 63, 64]


def test_nan_ignoring_option_leaves_the_rest_of_the_block_alone():
    x = md.random_rows(4, 64, seed=1)
    q0, s0 = md.encode(x)
    xn = x.clone()
    xn[2, 40] = float("nan")
    q1, s1 = md.encode(xn, ignore_nan=True)
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[2, 32:] = False
    assert torch.equal(q1[keep], q0[keep]) and (q1[2, 40] & 0x7F) == 0x7F
    x0 = x.clone()
    x0[2, 40] = 0.0
    qz, sz = md.encode(x0)
    keep[2, 32:] = True
    keep[2, 40] = False
    assert torch.equal(q1[keep], qz[keep]) and torch.equal(s1, sz)
    # the default propagates it: scale 2^126, everything else flushed
    q2, s2 = md.encode(xn)
    assert int(s2[2, 1]) == 253 and bool(((q2[2, 32:] & 0x7F) == 0)[torch.arange(32) != 8].all())
    assert torch.equal(s2[:2], s0[:2])


# ---- the designs --------------------------------------------------------------------------------------------------
def test_edge_blocks_are_bf16_exact_and_reach_every_edge():
    x = md.edge_blocks()
    assert torch.equal(bf16_round(x), x) and bool(torch.isfinite(x).all())
    nb = x.shape[1] // 32
    blocks = x.reshape(-1, 32)[:len(md.EDGE_NAMES)]
    by = dict(zip(md.EDGE_NAMES, blocks))
    q, s = md.encode(x)
    e = (s.reshape(-1)[:len(md.EDGE_NAMES)].to(torch.int32) - 127).tolist()
    ex = dict(zip(md.EDGE_NAMES, e))
    for k in (-126, -110, -20, -1, 0, 3, 40, 118):
        assert float(by[f"max448_k{k}"].abs().max()) == 448.0 * 2.0 ** k
        assert (ex[f"max446_k{k}"], ex[f"max448_k{k}"], ex[f"max450_k{k}"]) == (k, k, min(k + 1, 126))
    # the clamp: block exponents reach -126 with maxima below 448 * 2^-126, on bf16-subnormal inputs
    for n in ("clamp_max_2^-120", "clamp_max_subnormal", "clamp_min_subnormal", "clamp_448*2^-127"):
        assert ex[n] == -126 and float(by[n].abs().max()) < 448.0 * 2.0 ** -126
        assert bool(((by[n] != 0) & (by[n].abs() < 2.0 ** -126)).any()), "no bf16-subnormal input"
    assert ex["zeros"] == ex["neg_zeros"] == -126 and min(e) == -126 and max(e) >= 119
    qb = dict(zip(md.EDGE_NAMES, q.reshape(-1, 32)[:len(md.EDGE_NAMES)]))
    assert set(qb["zeros"].tolist()) | set(qb["neg_zeros"].tolist()) == {0x00, 0x80}
    assert float(by["bf16_max"].abs().max()) == float(torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16))
    # the subnormal sweep separates the cases: every subnormal code and zero appear, ties round to even both ways, and
    # 2^-10 (1 + 2^-7) rounds up to 2^-9 under a maximum of 448 but to 0 under 450
    codes = set((qb["max448_k0"] & 0x7F).tolist())
    assert set(range(0, 9)) <= codes
    v = by["max448_k0"].abs()
    pay = qb["max448_k0"] & 0x7F
    for m in range(8):
        tie = (2 * m + 1) * 2.0 ** -10
        assert int(pay[v == tie][0]) == (m if m % 2 == 0 else m + 1), m
    above = 2.0 ** -10 * (1 + 2.0 ** -7)
    assert int(pay[v == above][0]) == 1
    assert int((qb["max450_k0"] & 0x7F)[by["max450_k0"].abs() == above][0]) == 0
    # the maximum visits all four lanes of a quad (positions 0-7, 8-15, 16-23, 24-31)
    lanes = {int(b.abs().argmax()) // 8 for b in blocks}
    assert lanes == {0, 1, 2, 3}
    # any shape tiles the list
    y = md.edge_blocks(33, 96)
    assert y.shape == (33, 96) and torch.equal(y.reshape(-1, 32)[:nb], x.reshape(-1, 32)[:nb])


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (65, 192, 320), (300, 320, 1536)])
def test_gemm_designs_are_exact_and_within_bounds(M, N, K):
    for f in (md.integer_case, md.wide_scale_case):
        x, w, ref = f(M, N, K, seed=2)
        assert torch.equal(bf16_round(x), x) and torch.equal(bf16_round(w), w)
        assert float((x.abs().double() @ w.abs().double().t()).max()) < 2 ** 24  # exact in fp32, in any order
        # the quantiser holds them exactly
        assert torch.equal(md.decode(*md.encode(x)), x.double()) and torch.equal(md.decode(*md.encode(w)), w.double())
    x, w, ref = md.wide_scale_case(M, N, K, seed=2)
    _, sa = md.encode(x)
    e = sa.to(torch.int32) - 127
    if K >= 128:
        assert int(e.max()) - int(e.min()) >= 80, "block exponents do not span the wide range"
        assert bool((x.reshape(M, -1, 32) != 0).any(-1).all()), "a K block without a non-zero element"
    assert float(ref.abs().max()) <= 128 * 16 and torch.equal(bf16_round(ref).double(), ref)


@pytest.mark.parametrize("kind", ["bias", "resid", "gelu", "swiglu"])
def test_epilogue_designs_are_exact(kind):
    M, N, K = 65, 192, 320
    c = md.epilogue_case(kind, M, N, K, seed=1)
    assert torch.equal(bf16_round(c["x"]), c["x"]) and torch.equal(bf16_round(c["w"]), c["w"])
    want = c["want"]
    if kind == "resid":
        assert torch.equal(bf16_round(c["want_nogamma"]), c["want_nogamma"])
    if kind == "gelu":
        v = c["pre"]
        assert bool(((v == 0) | (v.abs() >= 8)).all()) and bool((v <= -8).any()) and bool((v >= 8).any())
        blocks = v.reshape(M, N // 32, 32)
        assert bool((blocks[:, :-1] >= 8).any(-1).all()) and bool((blocks[:, -1] == 0).all())
        # float64 erf-GELU agrees to well inside the e4m3 grid: the tail is 3.4e-8
        ref = torch.nn.functional.gelu(v.double())
        assert float((ref - want.double()).abs().max()) < 1e-6
        q, s = md.encode(want)
        assert bool((q[v <= -8] == 0x80).all()) and bool((s[:, -1] == 1).all())
    elif kind == "swiglu":
        g, u = c["pre"], c["pre_u"]
        assert bool(((g == 0) | (g >= 32) | (g <= -128)).all()) and float(u.abs().max()) <= 3
        assert all(bool(m.any()) for m in (g == 0, g >= 32, g <= -128))
        ref = torch.nn.functional.silu(g.double()) * u.double()
        assert float((ref - want.double()).abs().max()) < 1e-9
        assert bool((want == 0).reshape(M, N // 32, 32)[:, -1].all())
        # the packed weight puts x1 / x2 rows in alternating blocks of 32
        P = swiglu_perm(2 * N)
        assert torch.equal(c["w"][P].reshape(-1, 2, 32, K)[:, 0].reshape(N, K), c["w"][:N])
    if kind != "gelu":
        assert torch.equal(bf16_round(want), want)
    if kind in ("gelu", "swiglu"):
        # what the MX output feeds to a second GEMM gives an exact integer product
        y = md.decode(*md.encode(want)) @ md.second_weight(64, N, seed=3).double().t()
        assert torch.equal(bf16_round(y).double(), y)


# ---- the checks bite ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quant_case():
    x = md.edge_blocks(65, 96)
    return x, md.encode(x, ignore_nan=True)


def _quant_check(quant_case, bug=None):
    x, (wq, ws) = quant_case
    q, flat = md.model_quantize(x, bug=bug)
    md.check_bytes_equal(q, md.gather_scales(flat, *x.shape), wq, ws, str(bug))
    assert bool((flat[md.unwritten_mask(*x.shape)] == 0).all()), f"{bug}: a byte outside the valid slots was written"


def test_clean_quantiser_model_passes(quant_case):
    _quant_check(quant_case)
    x = md.random_rows(70, 96, seed=5)
    _quant_check((x, md.encode(x)))


@pytest.mark.parametrize("bug", md.BUGS_QUANT)
def test_each_quantiser_bug_is_rejected(quant_case, bug):
    with pytest.raises(AssertionError, match=bug):
        _quant_check(quant_case, bug)


def test_dequantise_round_trip_misses_a_layout_error_the_raw_bytes_catch(quant_case):
    """the reason for comparing raw bytes: a dequantiser that shares the quantiser's wrong slot order gives the same
    values back"""
    x, (wq, ws) = quant_case
    q, flat = md.model_quantize(x, bug="pair_swapped")
    same_wrong_layout = md.gather_scales(flat, *x.shape, bug="pair_swapped")
    assert torch.equal(md.decode(q, same_wrong_layout), md.decode(wq, ws))
    assert not torch.equal(md.gather_scales(flat, *x.shape), ws)


@pytest.fixture(scope="module")
def gemm_cases():
    out = {}
    for name, f in (("integer", md.integer_case), ("wide", md.wide_scale_case)):
        x, w, ref = f(129, 192, 320, seed=4)
        out[name] = (md.model_quantize(x), md.model_quantize(w), ref)
    return out


@pytest.mark.parametrize("name", ["integer", "wide"])
def test_clean_gemm_model_is_exact(gemm_cases, name):
    (aq, asf), (wq, wsf), ref = gemm_cases[name]
    assert torch.equal(md.model_linear_mx(aq, asf, wq, wsf), ref)


@pytest.mark.parametrize("bug", md.BUGS_GEMM)
@pytest.mark.parametrize("name", ["integer", "wide"])
def test_each_gemm_scale_bug_is_rejected(gemm_cases, name, bug):
    (aq, asf), (wq, wsf), ref = gemm_cases[name]
    got = md.model_linear_mx(aq, asf, wq, wsf, bug)
    assert not torch.equal(got, ref), bug
    if name == "wide" and bug == "neighbour_scale":
        # off by a large power of two, not by at most 4 as on the {0, 1, 2} shifts
        nz = (ref != 0) & (got != 0)
        assert float((got[nz] / ref[nz]).abs().log2().abs().max()) > 20


def test_wide_scales_separate_a_neighbour_scale_the_small_shifts_can_hide():
    """where both rows carry the same shift in neighbouring blocks the integer case cannot see the exchange at all; the
    wide case never has equal neighbours"""
    x, w, ref = md.wide_scale_case(65, 64, 384, seed=9)
    _, sa = md.encode(x)
    nzb = (x.reshape(65, -1, 32) != 0).any(-1)
    assert bool(nzb.all()) and bool((sa[:, 0::2] != sa[:, 1::2]).all())


@pytest.mark.parametrize("kind", ["gelu", "swiglu"])
def test_clean_epilogue_model_passes_and_each_bug_is_rejected(kind):
    M, N = 65, 192
    c = md.epilogue_case(kind, M, N, 192, seed=6)
    wq, ws = md.encode(c["want"])
    q, flat = md.model_epilogue_mx(c, kind)
    md.check_bytes_equal(q, md.gather_scales(flat, M, N), wq, ws, "clean")
    for bug in md.BUGS_EPI:
        if bug == "no_fold" and kind == "gelu":
            continue
        q, flat = md.model_epilogue_mx(c, kind, bug)
        with pytest.raises(AssertionError, match=bug):
            md.check_bytes_equal(q, md.gather_scales(flat, M, N), wq, ws, bug)


# ---- LayerNorm to MX ----------------------------------------------------------------------------------------------
_ln_cache = {}


def _ln(M, D):
    if (M, D) not in _ln_cache:
        _ln_cache[(M, D)] = md.ln_mx_case(M, D)
    return _ln_cache[(M, D)]


def test_noise_constant_covers_the_fp32_model():
    """NOISE_ULPS = 4 x the largest float64-versus-fp32-model difference over the designed cases (in fp32 ulps of S)"""
    worst = max(md.measured_noise_ulps(_ln(M, D)) for M in LN_ROWS for D in LN_DIMS)
    print(f"largest |float64 - fp32 model| = {worst:.3f} ulp32(S); NOISE_ULPS = {md.NOISE_ULPS}")
    assert worst <= md.MEASURED_ULPS <= worst + 0.01 and md.NOISE_ULPS == 4 * md.MEASURED_ULPS


@pytest.mark.parametrize("D", LN_DIMS)
@pytest.mark.parametrize("M", LN_ROWS)
def test_ln_reference_alone_stays_inside_the_exclusion_cap(M, D):
    c = _ln(M, D)
    x = c["x"]
    assert torch.equal(bf16_round(x), x) and float(x.abs().max()) <= 200
    assert bool((c["gamma"].log2() == c["gamma"].log2().round()).all()) and bool(((c["beta"] * 8) % 1 == 0).all())
    # the float64 reference through the oracle, and the fp32 model: no byte differs, nothing is excluded
    q, s = md.encode(c["ref"].float())
    n = md.check_mx_bytes(q, s, c["ref"], md.ln_noise(c), f"reference {M}x{D}")
    assert n <= M * D / 2000
    mq, ms = md.model_ln_mx(c)
    assert md.check_mx_bytes(mq, ms, c["ref"], md.ln_noise(c), f"model {M}x{D}") == n
    print(f"{M}x{D}: {n} excluded, model differs from the reference on {int((mq != q).sum())} bytes")
    if M >= 10:
        const = c["const"]
        assert int(const.sum()) == M // 10
        assert torch.equal(c["ref"][const].float(), c["beta"].expand(int(const.sum()), -1))
        assert float(md.ln_noise(c)[const].max()) == 0.0


@pytest.mark.parametrize("bug", md.BUGS_LN + ("floor_exp", "trunc", "amax8", "amax16"))
def test_each_layernorm_mx_bug_is_rejected(bug):
    c = _ln(130, 544)
    with pytest.raises(AssertionError, match=bug):
        md.check_mx_bytes(*md.model_ln_mx(c, bug), c["ref"], md.ln_noise(c), bug)


def test_exclusion_cap_is_enforced():
    """a noise large enough to cover the grid excludes everything, and the check then fails on the cap, not passes"""
    c = _ln(5, 96)
    q, s = md.model_ln_mx(c)
    with pytest.raises(AssertionError, match="within the noise"):
        md.check_mx_bytes(q, s, c["ref"], torch.full_like(c["ref"], 1.0), "cap")
