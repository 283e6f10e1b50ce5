"""GPU: the MX-fp8 path (BASELINE config 5) against exact references, byte for byte.

  a. mx_quant_kernel        raw payload and scale bytes == the oracle's raw encoding (oracle/mx_designs.py) on edge_blocks
                            and random rows; no byte outside the valid (row, block) slots is written; then dequantize()
  b. ln_mx_kernel           designed rows (ln_mx_case): check_mx_bytes against the float64 LayerNorm, constant rows exact;
                            the same through the SAM window partition
  c. gemm_mx_kernel, bf16   integer and wide-scale operands at 1 .. 6 and 24 K units (ring depth 3), M = 1 .. 300; every
                            bf16 epilogue on all three tile variants, bit-exact on integer / dyadic data
  d. gemm_mx_kernel, MX out gelu_exact_case / swiglu_exact_case: bytes == the oracle quantiser of exact values
  e. padding                scale bytes outside the valid rows do not reach a valid output row
  f. non-finite inputs      what a NaN or an Inf element does to its block and to a GEMM (pinned, see the docstrings)

tests/test_mx_gates_cpu.py shows on the CPU that each check used here rejects the bugs it is aimed at.  Every comparison
is on bit patterns; the one tolerance, NOISE_ULPS of check_mx_bytes in (b), is derived in oracle/mx_designs.py."""
import pytest
import torch

import sam_ops_ref as sr
from fixtures import ops  # noqa: F401
from ops_checks import bf
from oracle import mx_designs as md
from oracle import mx_oracle as mx

pytestmark = pytest.mark.gpu

GUARD = 256      # guard bytes either side of a payload or a scale array (keeps the 16-byte alignment)
QFILL = 0xA5     # prefill of payloads and guards
SENTINEL = 0x5A  # prefill of scale arrays: no test produces the scale 2^-37
EPS = 1e-6


def _guarded_mx(ops, rows, K, sfill=SENTINEL):
    """(MxTensor, payload allocation, scale allocation): both arrays sit between GUARD prefilled bytes"""
    nq, ns = rows * K, md.mx_rows_pad(rows) * (K // 32)
    qw = torch.full((nq + 2 * GUARD,), QFILL, dtype=torch.uint8, device="cuda")
    sw = torch.full((ns + 2 * GUARD,), sfill, dtype=torch.uint8, device="cuda")
    return ops.MxTensor(qw[GUARD:GUARD + nq].view(rows, K), sw[GUARD:GUARD + ns]), qw, sw


def _check_guarded(t, qw, sw, what, sfill=SENTINEL, valid_rows=None):
    """guards intact, and every scale byte that is no valid (row, block) slot still holds its prefill"""
    qw, sw = qw.cpu(), sw.cpu()
    assert bool((qw[:GUARD] == QFILL).all()) and bool((qw[-GUARD:] == QFILL).all()), f"{what}: payload guard overwritten"
    assert bool((sw[:GUARD] == sfill).all()) and bool((sw[-GUARD:] == sfill).all()), f"{what}: scale guard overwritten"
    rows, K = t.q.shape
    rest = md.unwritten_mask(rows, K)
    if valid_rows is not None:
        rest[:] = True
        rest[md.mx_scale_offsets(rows, valid_rows, K).reshape(-1)] = False
    assert bool((sw[GUARD:-GUARD][rest] == sfill).all()), f"{what}: a scale byte outside the valid slots was written"


def _raw(t):
    """(payload bytes [rows, K], scale bytes [rows, K/32]) of an MxTensor, on the CPU"""
    rows, K = t.q.shape
    return t.q.cpu(), md.gather_scales(t.scales, rows, K)


def _quant(ops, x, sfill=None):
    """x (float, bf16-exact) quantised on the GPU; sfill: the value of the scale bytes outside the valid rows"""
    t = ops.mx_quantize(bf(x).cuda())
    if sfill is not None:
        rest = md.unwritten_mask(*x.shape).cuda()
        t.scales[rest] = sfill
    return t


# ---- a. the quantiser, raw ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 96, 544, 2048])
@pytest.mark.parametrize("rows", [1, 31, 33, 64, 65, 255, 257, 513])
def test_quantiser_raw_bytes(ops, rows, K):
    for name, x in (("edge_blocks", md.edge_blocks(rows, K)), ("random", md.random_rows(rows, K, seed=rows + K))):
        what = f"{name} {rows}x{K}"
        t, qw, sw = _guarded_mx(ops, rows, K)
        ops.mx_quantize(bf(x).cuda(), out=t)
        torch.cuda.synchronize()
        want_q, want_s = md.encode(x)
        md.check_bytes_equal(*_raw(t), want_q, want_s, what)
        assert torch.equal(md.exact_scale_exponent(x.reshape(rows, -1, 32).abs().amax(-1)), want_s.to(torch.int32) - 127)
        _check_guarded(t, qw, sw, what)
        # and the dequantiser on those bytes: the oracle's, bit for bit
        got = t.dequantize().cpu()
        want = mx.mx_dequantize(want_q.view(torch.float8_e4m3fn), want_s.to(torch.int32) - 127)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{what}: dequantize"


# ---- b. LayerNorm to MX -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 96, 512, 544, 1536, 2048])
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_layernorm_mx_designed_rows(ops, rows, D):
    c = md.ln_mx_case(rows, D)
    t, qw, sw = _guarded_mx(ops, rows, D)
    ops.layernorm_mx(bf(c["x"]).cuda(), c["gamma"].cuda(), c["beta"].cuda(), EPS, out=t)
    torch.cuda.synchronize()
    q, s = _raw(t)
    n = md.check_mx_bytes(q, s, c["ref"], md.ln_noise(c), f"layernorm_mx {rows}x{D}")
    print(f"layernorm_mx {rows}x{D}: {n} of {rows * D} elements excluded")
    _check_guarded(t, qw, sw, f"layernorm_mx {rows}x{D}")
    const = c["const"]
    if const.any():  # x - mean = 0: the output is beta exactly, whatever rstd is
        wq, ws = md.encode(c["beta"].expand(int(const.sum()), -1))
        md.check_bytes_equal(q[const], s[const], wq, ws, f"constant rows {rows}x{D}")


@pytest.mark.parametrize("batch,g,ws,D", [(2, 10, 4, 544)])
def test_layernorm_mx_window_designed_rows(ops, batch, g, ws, D):
    """border windows (g = 10, ws = 4: 12 x 12 windowed rows per image): the partitioned rows hold the bytes of the plain
    kernel's token rows, which pass check_mx_bytes; padding rows are not written"""
    idx, valid = sr.window_index(batch, g, ws)
    rows, wrows = batch * g * g, sr.window_rows(batch, g, ws)
    c = md.ln_mx_case(rows, D)
    x, gamma, beta = bf(c["x"]).cuda(), c["gamma"].cuda(), c["beta"].cuda()
    q, s = _raw(ops.layernorm_mx(x, gamma, beta, EPS))
    n = md.check_mx_bytes(q, s, c["ref"], md.ln_noise(c), "layernorm_mx (token order)")
    print(f"layernorm_mx_window {rows}x{D}: {n} of {rows * D} elements excluded")
    t, qw, sw = _guarded_mx(ops, wrows, D)
    ops.layernorm_mx_window(x, gamma, beta, EPS, batch, g, ws, out=t)
    torch.cuda.synchronize()
    wq, wsb = _raw(t)
    md.check_bytes_equal(wq[valid], wsb[valid], q[idx[valid]], s[idx[valid]], "windowed rows")
    assert bool((wq[~valid] == QFILL).all()), "a padding row's payload was written"
    _check_guarded(t, qw, sw, "layernorm_mx_window", valid_rows=torch.nonzero(valid).reshape(-1))


# ---- c. the GEMM, bf16 out ----------------------------------------------------------------------------------------
KS = (64, 128, 192, 256, 320, 384, 1536)  # 1 .. 6 K units around the ring depth of 3, and 24
MS = (1, 63, 65, 129, 300)
NS = (64, 192, 320)
GEMM_CROSS = [(v, MS[(i + 2 * v) % 5], NS[(i + v) % 3], K) for v in (0, 1, 2) for i, K in enumerate(KS)]


def test_gemm_cross_is_representative():
    for v in (0, 1, 2):
        mine = [c for c in GEMM_CROSS if c[0] == v]
        assert {c[1] for c in mine} == set(MS) and {c[2] for c in mine} == set(NS) and {c[3] for c in mine} == set(KS)


@pytest.mark.parametrize("variant,M,N,K", GEMM_CROSS)
def test_linear_mx_integer_and_wide_scale_exact(ops, variant, M, N, K):
    for name, f in (("integer", md.integer_case), ("wide", md.wide_scale_case)):
        x, w, ref = f(M, N, K, seed=M + N + K + variant)
        xq, wq = _quant(ops, x), _quant(ops, w)
        md.check_bytes_equal(*_raw(xq), *md.encode(x), f"{name} x")
        md.check_bytes_equal(*_raw(wq), *md.encode(w), f"{name} w")
        y = ops.linear_mx(xq, wq, variant=variant)
        md.check_exact_bf16_bits(y, ref.float(), f"{name} variant {variant} {M}x{N}x{K}")


EPI_SHAPES = ((65, 192, 192), (129, 320, 320), (300, 64, 384))


@pytest.mark.parametrize("kind", ["bias", "gelu", "resid", "resid_layerscale", "resid_in_place", "swiglu"])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_linear_mx_bf16_epilogues_exact(ops, variant, kind):
    from vdr import _lib as L

    base = kind.split("_")[0]
    M, N, K = EPI_SHAPES[(variant + len(kind)) % 3]
    c = md.epilogue_case(base, M, N, K, seed=10 * variant + len(kind))
    xq = _quant(ops, c["x"])
    what = f"{kind} variant {variant} {M}x{N}x{K}"
    if base == "swiglu":
        wp, bp = ops.pack_w12(c["w"], c["bias"])
        y = ops.linear_mx(xq, _quant(ops, wp), bias=bp.cuda(), epilogue=L.EPI_SWIGLU, variant=variant)
        assert tuple(y.shape) == (M, N)
        md.check_exact_bf16_bits(y, c["want"], what)  # signed zeros included
        return
    wq, b = _quant(ops, c["w"]), c["bias"].cuda()
    if base == "bias":
        md.check_exact_bf16_bits(ops.linear_mx(xq, wq, bias=b, variant=variant), c["want"], what)
    elif base == "gelu":
        y = ops.linear_mx(xq, wq, bias=b, epilogue=L.EPI_BIAS_GELU, variant=variant).cpu()
        neg = c["pre"] <= -8
        md.check_exact_bf16_bits(torch.where(neg, torch.zeros_like(y), y), torch.where(neg, torch.zeros_like(c["want"]), c["want"]), what)
        # v <= -8: one constant, bf16 of the polynomial's tail -5.7 * 2^Q(5.7) (v_exp_f32 is good to 1 ulp: within one
        # bf16 ulp of the float64 value)
        tail = y[neg].float()
        assert bool((tail == tail[0]).all()) and abs(float(tail[0]) / md.GELU_NEG_TAIL - 1.0) <= 2.0 ** -7, what
    else:
        r = bf(c["resid"]).cuda()
        gam = None if kind == "resid" else c["gamma"].cuda()
        want = c["want_nogamma"] if kind == "resid" else c["want"]
        out = r.clone() if kind == "resid_in_place" else None
        y = ops.linear_mx(xq, wq, bias=b, resid=out if out is not None else r, gamma=gam, epilogue=L.EPI_BIAS_RESID,
                          variant=variant, out=out)
        md.check_exact_bf16_bits(y, want, what)


# ---- d. the GEMM, MX out ------------------------------------------------------------------------------------------
MXO_M, MXO_N, MXO_K = (1, 65, 333), (64, 192, 512), (64, 192, 768)
MXO_CROSS = [(v, MXO_M[i], MXO_N[(i + v) % 3], MXO_K[(i + 2 * v) % 3]) for v in (0, 1, 2) for i in range(3)]


def _run_mx_out(ops, c, kind, variant, out, x_fill=None, w_fill=None):
    from vdr import _lib as L

    xq = _quant(ops, c["x"], x_fill)
    if kind == "gelu":
        return ops.linear_mx(xq, _quant(ops, c["w"], w_fill), bias=c["bias"].cuda(), epilogue=L.EPI_BIAS_GELU,
                             variant=variant, mx_out=True, out=out)
    wp, bp = ops.pack_w12(c["w"], c["bias"])
    return ops.linear_mx(xq, _quant(ops, wp, w_fill), bias=bp.cuda(), epilogue=L.EPI_SWIGLU, variant=variant,
                         mx_out=True, out=out)


@pytest.mark.parametrize("kind", ["gelu", "swiglu"])
@pytest.mark.parametrize("variant,M,N,K", MXO_CROSS)
def test_linear_mx_output_bytes_exact(ops, variant, M, N, K, kind):
    """N is the width of the MX output (the SwiGLU GEMM has 2 N packed columns).  Payload and scale bytes equal the
    oracle quantiser of the exact activation values, no exclusions; a second GEMM on them gives the exact integer product"""
    c = md.epilogue_case(kind, M, N, K, seed=100 * variant + M)
    what = f"{kind} MX out variant {variant} {M}x{N}x{K}"
    t, qw, sw = _guarded_mx(ops, M, N)
    _run_mx_out(ops, c, kind, variant, t)
    torch.cuda.synchronize()
    want_q, want_s = md.encode(c["want"])
    md.check_bytes_equal(*_raw(t), want_q, want_s, what)
    _check_guarded(t, qw, sw, what)
    if N % 64 == 0:  # (always: the consumer needs K % 64 == 0)
        w2 = md.second_weight(64, N, seed=N + variant)
        ref = md.decode(want_q, want_s) @ w2.double().t()
        assert float(ref.abs().max()) < 2 ** 15
        md.check_exact_bf16_bits(ops.linear_mx(t, _quant(ops, w2)), ref.float(), what + ": second GEMM")


# ---- e. padding does not leak -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,M,N,K", [(0, 65, 192, 192), (1, 300, 320, 128), (2, 129, 192, 384)])
def test_scale_padding_does_not_leak(ops, variant, M, N, K):
    """In a forward the scale arrays live in reused workspace: the bytes of the rows between M and the padded row count
    (and past N for the weight) hold anything.  M is no multiple of 64 and N (a multiple of 64 by the GEMM's contract) is no
    multiple of the tile width: rows and columns of the last tiles read those bytes.  With them set to 0x00, 0x7F and 0xFF
    in turn, on A, W and the MX output, the valid rows are bitwise the same"""
    x, w, ref = md.wide_scale_case(M, N, K, seed=variant)
    results, mx_results = [], {"gelu": [], "swiglu": []}
    cg = {k: md.epilogue_case(k, M, N, K, seed=7 + variant) for k in mx_results}
    for fill in (0x00, 0x7F, 0xFF):
        results.append(ops.linear_mx(_quant(ops, x, fill), _quant(ops, w, fill), variant=variant).cpu())
        for kind in mx_results:
            t, qw, sw = _guarded_mx(ops, M, N, sfill=fill)
            _run_mx_out(ops, cg[kind], kind, variant, t, fill, fill)
            torch.cuda.synchronize()
            _check_guarded(t, qw, sw, f"{kind} fill {fill:#x}", sfill=fill)
            mx_results[kind].append(_raw(t))
    md.check_exact_bf16_bits(results[0], ref.float(), "fill 0x00")
    for y in results[1:]:
        assert torch.equal(y.view(torch.int16), results[0].view(torch.int16)), "scale padding reached a valid output row"
    for kind, rs in mx_results.items():
        md.check_bytes_equal(*rs[0], *md.encode(cg[kind]["want"]), f"{kind} fill 0x00")
        for q, s in rs[1:]:
            md.check_bytes_equal(q, s, *rs[0], f"{kind}: scale padding reached a valid output row")


# ---- f. non-finite inputs -----------------------------------------------------------------------------------------
def test_nan_element_in_the_quantiser(ops):
    """Pinned: the block maximum is taken with fmaxf, which drops a NaN.  The NaN element becomes the e4m3 NaN (0x7f or
    0xff) and dequantises to NaN; every other element of its block, and the block's scale, are what they are with the NaN
    replaced by 0 (mx_oracle's ignore_nan option).  A block of NaN only has scale 2^-126"""
    x = md.random_rows(5, 96, seed=3)
    x[2, 40] = float("nan")
    x[4, 64:] = float("nan")
    t = ops.mx_quantize(bf(x).cuda())
    q, s = _raw(t)
    want_q, want_s = md.encode(x, ignore_nan=True)
    nan = torch.isnan(x)
    assert bool(((q[nan] & 0x7F) == 0x7F).all()), "a NaN element was laundered into a finite e4m3 value"
    md.check_bytes_equal(torch.where(nan, want_q, q), s, want_q, want_s, "NaN-ignoring oracle")
    assert int(s[4, 2]) == 1
    d = t.dequantize().cpu()
    assert torch.equal(torch.isnan(d), nan) and bool(torch.isfinite(d[~nan]).all())


def test_inf_element_in_the_quantiser(ops):
    """Pinned: an Inf element makes the block maximum Inf, so the scale exponent clamps to 126 (byte 253); Inf * 2^-126 is
    Inf, which the conversion turns into the e4m3 NaN (e4m3fn has no infinity): the element dequantises to NaN.  The rest of
    the block is multiplied by 2^-126 and flushes to signed zeros (all of it, for |x| < 2^116).  Other blocks are untouched"""
    x = md.random_rows(5, 96, seed=4)
    x0 = x.clone()
    x[1, 7], x[3, 70] = float("inf"), float("-inf")
    t = ops.mx_quantize(bf(x).cuda())
    q, s = _raw(t)
    inf = torch.isinf(x)
    d = t.dequantize().cpu()
    assert bool((~torch.isfinite(d[inf])).all()), "an Inf element dequantises to a finite value"
    want_q, want_s = md.encode(x)
    assert int(want_s[1, 0]) == 253 and int(want_s[3, 2]) == 253
    md.check_bytes_equal(torch.where(inf, want_q, q), s, want_q, want_s, "Inf block")
    assert bool(((q[inf] & 0x7F) == 0x7F).all())
    blk = torch.zeros_like(inf)
    blk[1, :32], blk[3, 64:] = True, True
    assert bool(((q[blk & ~inf] & 0x7F) == 0).all())
    q0, s0 = md.encode(x0)
    assert torch.equal(q[~blk], q0[~blk])


def test_nan_row_in_layernorm_mx(ops):
    """Pinned: a NaN in a row makes its mean NaN, so every element of that row is the e4m3 NaN (block maxima 0 under fmaxf:
    scale 2^-126); other rows are bitwise unchanged"""
    c = md.ln_mx_case(5, 96)
    x = c["x"].clone()
    x[2, 50] = float("nan")
    g, b = c["gamma"].cuda(), c["beta"].cuda()
    q0, s0 = _raw(ops.layernorm_mx(bf(c["x"]).cuda(), g, b, EPS))
    q, s = _raw(ops.layernorm_mx(bf(x).cuda(), g, b, EPS))
    keep = torch.arange(5) != 2
    md.check_bytes_equal(q[keep], s[keep], q0[keep], s0[keep], "rows without the NaN")
    assert bool(((q[2] & 0x7F) == 0x7F).all()) and bool((s[2] == 1).all())


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_nan_element_in_linear_mx(ops, variant):
    """Pinned: an e4m3 NaN in row r of A makes output row r NaN in every column (bias epilogue, bf16 out) and every byte of
    row r the e4m3 NaN (SwiGLU epilogue, MX out: silu propagates NaN); all other rows are bitwise unchanged.  (The erf-GELU
    epilogue is the documented exception, csrc/vdr_dev.h: v_min / v_max drop the NaN, so a NaN accumulator comes out as the
    negative tail.)"""
    from vdr import _lib as L

    M, N, K, r = 130, 192, 192, 77
    c = md.epilogue_case("swiglu", M, N, K, seed=variant)
    x = c["x"].clone()
    x[r, 100] = float("nan")
    wp, bp = ops.pack_w12(c["w"], c["bias"])
    wq, bias = _quant(ops, wp), bp.cuda()
    keep = torch.arange(M) != r
    y0 = ops.linear_mx(_quant(ops, c["x"]), wq, bias=bias, variant=variant).cpu()
    y = ops.linear_mx(_quant(ops, x), wq, bias=bias, variant=variant).cpu()
    assert torch.equal(y[keep].view(torch.int16), y0[keep].view(torch.int16)), "a row without the NaN changed"
    assert bool(torch.isnan(y[r]).all()) and bool(torch.isfinite(y0).all())
    q0, s0 = _raw(ops.linear_mx(_quant(ops, c["x"]), wq, bias=bias, epilogue=L.EPI_SWIGLU, variant=variant, mx_out=True))
    q, s = _raw(ops.linear_mx(_quant(ops, x), wq, bias=bias, epilogue=L.EPI_SWIGLU, variant=variant, mx_out=True))
    md.check_bytes_equal(q[keep], s[keep], q0[keep], s0[keep], "MX out: rows without the NaN")
    assert bool(((q[r] & 0x7F) == 0x7F).all()) and bool((s[r] == 1).all())
