"""GPU, through the C ABI: the SAM-only device paths, each against an exact reference.

  a. vdr_op_layernorm_window     -- layernorm_kernel with win_ws / win_g: valid windowed rows are bitwise vdr_op_layernorm's,
                                    padding rows and guard rows keep their canary; designed rows whose signs spell the token number
  b. vdr_op_layernorm_mx_window  -- ln_mx_kernel with win_ws / win_g: dequantised valid rows bitwise vdr_op_layernorm_mx's,
                                    padding rows 0; no byte of a padding row or past the windowed rows is written
  c. vdr_op_linear_window        -- epilogue_resid_impl<WIN = true> on integer data, every tile variant: bit-exact against a
                                    float64 matmul scattered through the checked index (tests/sam_ops_ref.py)
  d. the same on real-valued data: bitwise vdr_op_linear (VDR_EPI_BIAS_RESID) on the valid rows in token order
  e. the LayerNorm partials through the window: float64 sums of the stored outputs within the fp32 summation bound, bitwise
     vdr_op_linear_ln_stats's, nothing written past the token rows, NaN padding rows add nothing
  f. vdr_op_im2col3              -- bitwise F.unfold in tap-major order; the composed neck convolution exact on integers

Every comparison is on bit patterns (int16 / int32 views, torch.equal); the one bound, in (e), is derived there.
"""
import pytest
import torch

import sam_ops_ref as sr
from fixtures import ops  # noqa: F401
from ops_checks import bf

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A  # int16 pattern of the prefilled outputs and guard rows (as bf16: 1.5e16, no value any test produces)
GUARD = 5        # guard rows before and after an output
ALL_VARIANTS = (0, 22, 23, 24, 25, 26, 27, 28, 29)  # 0: what the forward picks for the out-projection; ring3, ring3k (25), ring4
EPS = 1e-6


def _bits(t):
    """bit patterns of a bf16 (int16) or fp32 (int32) tensor, on the CPU"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _guarded(rows, width, device="cuda"):
    """(whole, body): an int16 allocation of GUARD + rows + GUARD rows filled with the canary, and its middle as bf16"""
    whole = torch.full((rows + 2 * GUARD, width), CANARY, dtype=torch.int16, device=device)
    return whole, whole[GUARD:GUARD + rows].view(torch.bfloat16)


def _guards_intact(whole):
    w = whole.cpu()
    return bool((w[:GUARD] == CANARY).all()) and bool((w[-GUARD:] == CANARY).all())


_geo_cache = {}


def _geo(batch, g, ws):
    key = (batch, g, ws)
    if key not in _geo_cache:
        idx, valid = sr.window_index(batch, g, ws)
        _geo_cache[key] = (idx, valid, sr.token_to_window(batch, g, ws))
    return _geo_cache[key]


# ---- a. LayerNorm into window-partition order ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 192, 768, 1280])
@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_layernorm_window_is_layernorm_in_partition_order(ops, batch, g, ws, D):
    idx, valid, _ = _geo(batch, g, ws)
    gen = torch.Generator().manual_seed(1000 * g + 10 * ws + D)
    x = bf(torch.randn(batch * g * g, D, generator=gen) * 1.7 + 0.3).cuda()
    gamma = (torch.randn(D, generator=gen) * 0.5 + 1.0).cuda()
    beta = (torch.randn(D, generator=gen) * 0.3).cuda()
    want = _bits(ops.layernorm(x, gamma, beta, EPS))
    whole, body = _guarded(sr.window_rows(batch, g, ws), D)
    ops.layernorm_window(x, gamma, beta, EPS, batch, g, ws, out=body)
    torch.cuda.synchronize()
    got = _bits(body)
    assert torch.equal(got[valid], want[idx[valid]])
    assert bool((got[~valid] == CANARY).all()), "a padding row was written"
    assert _guards_intact(whole)


@pytest.mark.parametrize("D", [64, 1280])
@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_layernorm_window_rows_spell_their_token_number(ops, batch, g, ws, D):
    """Independent of vdr_op_layernorm: the signs of a normalised sam_ops_ref.token_code_rows row are its token number."""
    idx, valid, _ = _geo(batch, g, ws)
    x = bf(sr.token_code_rows(batch * g * g, D)).cuda()
    whole, body = _guarded(sr.window_rows(batch, g, ws), D)
    ops.layernorm_window(x, torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"), EPS, batch, g, ws, out=body)
    torch.cuda.synchronize()
    y = body.cpu()
    assert torch.equal(sr.decode_token_code(y[valid].float(), D), idx[valid])
    # and the values: (x - mean) * rsqrt(1 + eps) with |x - mean| = 1 is one number, up to its sign
    mag = y[valid].float().abs()
    assert bool((mag == mag[0, 0]).all()) and abs(float(mag[0, 0]) - 1.0) <= 2.0 ** -8
    assert bool((_bits(body)[~valid] == CANARY).all()) and _guards_intact(whole)


# ---- b. the same with MX-fp8 output -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 768, 1280])
@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_layernorm_mx_window(ops, batch, g, ws, D):
    idx, valid, _ = _geo(batch, g, ws)
    rows = sr.window_rows(batch, g, ws)
    gen = torch.Generator().manual_seed(2000 * g + 10 * ws + D)
    x = bf(torch.randn(batch * g * g, D, generator=gen) * 1.7 + 0.3).cuda()
    gamma = (torch.randn(D, generator=gen) * 0.5 + 1.0).cuda()
    beta = (torch.randn(D, generator=gen) * 0.3).cuda()
    want = _bits(ops.layernorm_mx(x, gamma, beta, EPS).dequantize())
    # zeroed payload and scales, as the forward prepares them
    t = ops.layernorm_mx_window(x, gamma, beta, EPS, batch, g, ws)
    assert t.scales.numel() == sr.mx_rows_pad(rows) * (D // 32)
    got = _bits(t.dequantize())
    assert torch.equal(got[valid], want[idx[valid]])
    assert bool((got[~valid] == 0).all()), "a padding row does not dequantise to +0"
    # 0xFF-prefilled buffers: only the bytes of valid rows change, and they become what they were above
    t2 = ops.MxTensor(torch.full_like(t.q, 0xFF), torch.full_like(t.scales, 0xFF))
    ops.layernorm_mx_window(x, gamma, beta, EPS, batch, g, ws, out=t2)
    torch.cuda.synchronize()
    q1, q2, s1, s2 = t.q.cpu(), t2.q.cpu(), t.scales.cpu(), t2.scales.cpu()
    assert torch.equal(q2[valid], q1[valid]) and bool((q2[~valid] == 0xFF).all())
    off = sr.mx_scale_offsets(rows, torch.nonzero(valid).reshape(-1), D).reshape(-1)
    assert torch.equal(s2[off], s1[off])
    rest = torch.ones(s2.numel(), dtype=torch.bool)
    rest[off] = False  # scale bytes of padding rows and of rows between the windowed row count and rows_pad
    assert int(rest.sum()) == (sr.mx_rows_pad(rows) - int(valid.sum())) * (D // 32)
    assert bool((s2[rest] == 0xFF).all()), "a scale byte outside the valid rows was written"
    assert bool((s1[rest] == 0).all())


# ---- c / d / e. the un-partitioning residual out-projection -------------------------------------------------------------
def _integer_case(batch, g, ws, N, K, seed, pad_value=100.0):
    """(c)'s operands on the CPU (float32 integers) and the float64 reference [batch*g*g, N]"""
    idx, valid, inv = _geo(batch, g, ws)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (sr.window_rows(batch, g, ws), K), generator=gen).float()
    x[~valid] = pad_value
    W = sr.sparse_sign_weight(N, K, gen)
    bias = torch.randint(-8, 9, (N,), generator=gen).float()
    resid = torch.randint(-64, 65, (batch * g * g, N), generator=gen).float()
    ref = resid.double() + x[inv].double() @ W.double().t() + bias.double()
    assert float(ref.abs().max()) <= 120
    return x, W, bias, resid, ref


def _run_window(ops, x, W, bias, resid, batch, g, ws, variant, in_place, part=None):
    """one launch inside guard rows; returns the output bits [batch*g*g, N] (CPU int16)"""
    whole, body = _guarded(resid.shape[0], resid.shape[1])
    if in_place:
        body.copy_(resid)
        ops.linear_window(x, W, bias, body, batch, g, ws, variant=variant, out=body, part=part)
    else:
        ops.linear_window(x, W, bias, resid, batch, g, ws, variant=variant, out=body, part=part)
    torch.cuda.synchronize()
    assert _guards_intact(whole), f"guard rows written (variant {variant}, in_place {in_place})"
    return _bits(body)


def _check_integer_case(ops, batch, g, ws, N, K, variants):
    x, W, bias, resid, ref = _integer_case(batch, g, ws, N, K, seed=g * 100 + ws + N)
    want = _bits(bf(ref.float()))
    assert torch.equal(bf(ref.float()).double(), ref)  # every expected output is a bf16 number
    xd, Wd, bd, rd = bf(x).cuda(), bf(W).cuda(), bias.cuda(), bf(resid).cuda()
    for v in variants:
        out = _run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=False)
        assert torch.equal(out, want), f"variant {v}: {int((out != want).any(1).sum())} of {want.shape[0]} rows differ"
        assert torch.equal(_run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=True), out), f"variant {v} in place"
    assert torch.equal(_bits(rd), _bits(bf(resid)))  # the out-of-place launches left the residual alone


@pytest.mark.parametrize("N,K", [(64, 64), (768, 768), (200, 128)])
@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_linear_window_exact_integers(ops, batch, g, ws, N, K):
    """x in [-3, 3], <= 16 entries of +-1 per W row (columns 0 and K - 1 always), bias in [-8, 8], resid in [-64, 64]:
    |y| <= 120, every output exact in bf16.  Padding rows of x hold 100 in every column: a leaked row is far outside the
    range.  (200, 128) has a ragged last column block."""
    _check_integer_case(ops, batch, g, ws, N, K, ALL_VARIANTS)


def test_linear_window_exact_integers_more_tiles_than_resident_workgroups(ops):
    """(4, 64, 14): 19 600 windowed rows x 768 columns -- 924 tiles of 128 x 128 (variant 28), 1842 of 64 x 128 (29): more
    than the chip holds resident workgroups of those ring4 variants, so the persistent ring4p kernel takes the launch.
    Nothing here asserts which kernel ran: the outputs are checked, as everywhere."""
    _check_integer_case(ops, 4, 64, 14, 768, 768, ALL_VARIANTS)


def _real_case(batch, g, ws, N, K, seed):
    idx, valid, inv = _geo(batch, g, ws)
    gen = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(sr.window_rows(batch, g, ws), K, generator=gen))
    W = bf(torch.randn(N, K, generator=gen) * 0.05)
    bias = torch.randn(N, generator=gen) * 0.2
    resid = bf(torch.randn(batch * g * g, N, generator=gen) * 1.5)
    return x, W, bias, resid, inv, valid


@pytest.mark.parametrize("batch,g,ws", sr.GEOMETRIES)
def test_linear_window_is_the_plain_residual_linear_on_the_valid_rows(ops, batch, g, ws):
    """Random bf16 x / W / resid, fp32 bias at (768, 768): every variant's rows are bitwise those vdr_op_linear
    (VDR_EPI_BIAS_RESID, the same variant) computes from the valid rows in token order."""
    from vdr import EPI_BIAS_RESID
    x, W, bias, resid, inv, _ = _real_case(batch, g, ws, 768, 768, seed=g * 10 + ws)
    xd, Wd, bd, rd = x.cuda(), W.cuda(), bias.cuda(), resid.cuda()
    x_tok = xd[inv.cuda()].contiguous()
    for v in ALL_VARIANTS:
        want = _bits(ops.linear(x_tok, Wd, bd, resid=rd, epilogue=EPI_BIAS_RESID, variant=v))
        assert torch.equal(_run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=False), want), f"variant {v}"
        assert torch.equal(_run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=True), want), f"variant {v} in place"


def _nan_part(N, tokens):
    return torch.full((N // 64, tokens + 37, 2), float("nan"), dtype=torch.float32, device="cuda")


def _check_part(part, out_bits, tokens, exact):
    """part [N/64, tokens + 37, 2] against float64 sums of the stored bf16 outputs.  fp32 summation of 64 terms in any
    order: |ds1| <= 63 u sum|r| (63 additions), |ds2| <= 64 u sum r^2 (63 additions plus the rounding of each fma; r^2 of
    a bf16 r is exact), u = 2^-24.  exact: integer data, both sums are integers below 2^24 -- no rounding at all."""
    p = part.cpu()
    assert bool(torch.isnan(p[:, tokens:]).all()), "a partial was written past the token rows"
    p = p[:, :tokens].double()
    assert not bool(torch.isnan(p).any()), "a valid row's partial was not written"
    r = out_bits.view(torch.bfloat16).double().reshape(tokens, -1, 64).permute(1, 0, 2)  # [N/64, tokens, 64]
    s1, s2, a1 = r.sum(-1), (r * r).sum(-1), r.abs().sum(-1)
    assert bool((p[..., 1] > 0).all()), "a valid row's partial is zero-filled"
    u = 0.0 if exact else 2.0 ** -24
    assert bool(((p[..., 0] - s1).abs() <= 63 * u * a1).all()), float(((p[..., 0] - s1).abs() / a1).max())
    assert bool(((p[..., 1] - s2).abs() <= 64 * u * s2).all()), float(((p[..., 1] - s2).abs() / s2).max())


@pytest.mark.parametrize("N", [64, 768])
@pytest.mark.parametrize("batch,g,ws", sr.PADDED_GEOMETRIES)
def test_linear_window_layernorm_partials(ops, batch, g, ws, N):
    """The (sum, sumsq) partials land at the un-partitioned row: against float64 sums of the stored outputs (bound in
    _check_part; bit-equal on integer data), bitwise the partials of the plain launch on the valid rows, rows past the
    tokens still NaN."""
    tokens = batch * g * g
    for v in (22, 26, 28):
        # integer data: exact
        x, W, bias, resid, ref = _integer_case(batch, g, ws, N, N, seed=g * 100 + ws + N + 1)
        xd, Wd, bd, rd = bf(x).cuda(), bf(W).cuda(), bias.cuda(), bf(resid).cuda()
        part = _nan_part(N, tokens)
        out = _run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=False, part=part)
        assert torch.equal(out, _bits(bf(ref.float())))
        _check_part(part, out, tokens, exact=True)
        # real-valued data: the summation bound, and the plain producer's bits
        x, W, bias, resid, inv, _ = _real_case(batch, g, ws, N, N, seed=g * 10 + ws + N)
        xd, Wd, bd, rd = x.cuda(), W.cuda(), bias.cuda(), resid.cuda()
        for in_place in (False, True):
            part = _nan_part(N, tokens)
            out = _run_window(ops, xd, Wd, bd, rd, batch, g, ws, v, in_place=in_place, part=part)
            _check_part(part, out, tokens, exact=False)
            plain = _nan_part(N, tokens)
            want = ops.linear_ln_stats(xd[inv.cuda()].contiguous(), Wd, bd, rd, plain, v)
            torch.cuda.synchronize()
            assert torch.equal(out, _bits(want)), f"variant {v}"
            assert torch.equal(_bits(part), _bits(plain)), f"variant {v}: partials differ from the plain launch's"


@pytest.mark.parametrize("N", [64, 768])
def test_linear_window_nan_padding_rows_add_nothing(ops, N):
    """Dropped rows are multiplied like any other; what they hold must reach neither an output nor a partial sum.  g = ws + 1:
    most windowed rows are padding, and padding and valid rows share 8-row groups of the epilogue.  (What keeps a dropped
    row out of the partials is the store guard: the DPP adds bring lane c8 == 0 the 8 lanes of its own row only, and with
    N % 64 == 0 those are all stored or all dropped, so the epilogue's `om < 0 ? 0` selects change no result.)"""
    batch, g, ws = 2, 15, 14
    tokens = batch * g * g
    x, W, bias, resid, inv, valid = _real_case(batch, g, ws, N, N, seed=77 + N)
    x_nan = x.clone()
    x_nan[~valid] = float("nan")
    Wd, bd, rd = W.cuda(), bias.cuda(), resid.cuda()
    for v in (22, 25, 26, 28, 29):
        res = []
        for xs in (x, x_nan):
            for in_place in (False, True):
                part = _nan_part(N, tokens)
                out = _run_window(ops, xs.cuda(), Wd, bd, rd, batch, g, ws, v, in_place=in_place, part=part)
                _check_part(part, out, tokens, exact=False)
                res.append((out, _bits(part)))
        for out, pb in res[1:]:
            assert torch.equal(out, res[0][0]) and torch.equal(pb, res[0][1]), f"variant {v}"


# ---- f. the neck's 3 x 3 im2col -----------------------------------------------------------------------------------------
IM2COL_GRIDS = [(1, 1), (3, 2), (2, 7), (3, 10), (1, 64)]


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("batch,g", IM2COL_GRIDS)
def test_im2col3_is_unfold_in_tap_major_order(ops, batch, g, C):
    gen = torch.Generator().manual_seed(g * 10 + C)
    x = bf(torch.randn(batch * g * g, C, generator=gen) * 3.0)
    flat = x.view(torch.int16).reshape(-1)
    n = flat.numel()
    flat[torch.randint(0, n, (n // 16 + 1,), generator=gen)] = -32768  # -0.0
    flat[torch.randint(0, n, (n // 16 + 1,), generator=gen)] = 0x7F7F  # the largest finite bf16
    flat[torch.randint(0, n, (n // 16 + 1,), generator=gen)] = -129    # 0xFF7F: the most negative finite bf16
    want = sr.im2col3_ref(x.view(torch.int16), batch, g)
    whole, body = _guarded(batch * g * g, 9 * C)
    ops.im2col3(x.cuda(), batch, g, out=body)
    torch.cuda.synchronize()
    assert torch.equal(_bits(body), want)
    assert _guards_intact(whole)


def test_im2col3_never_reads_the_neighbouring_image(ops):
    batch, g, C = 3, 7, 64
    x = torch.full((batch, g * g, C), 7.0)
    x[1] = 1.0
    col = ops.im2col3(bf(x).reshape(-1, C).cuda(), batch, g).float().cpu().reshape(batch, g, g, 9, C)
    mid = col[1]
    assert bool(((mid == 0) | (mid == 1)).all()), "image 1 holds a value of a neighbouring image"
    assert bool((mid[1:-1, 1:-1] == 1).all())
    # a border pixel: exactly the taps that fall outside the grid are zero
    assert torch.equal((mid[0, 0, :, 0] == 0).nonzero().reshape(-1), torch.tensor([0, 1, 2, 3, 6]))
    assert torch.equal((mid[-1, -1, :, 0] == 0).nonzero().reshape(-1), torch.tensor([2, 5, 6, 7, 8]))
    for b in (0, 2):
        assert bool(((col[b] == 0) | (col[b] == 7)).all())


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("batch,g", IM2COL_GRIDS)
def test_neck_conv3x3_through_im2col3_exact_integers(ops, batch, g, C):
    """The neck's second convolution as the forward composes it -- im2col3, then the linear on the tap-major weight -- on
    integers: x in [-4, 4], <= 32 taps of +-1 per output channel, |y| <= 128: bit-equal to float64 F.conv2d(padding = 1)."""
    from vdr import EPI_BIAS
    gen = torch.Generator().manual_seed(g * 10 + C + 5)
    x = torch.randint(-4, 5, (batch, g, g, C), generator=gen).float()
    Wt = sr.sparse_sign_weight(C, 9 * C, gen, nnz=32)                  # [C_out, (ky*3 + kx)*C_in + c]
    Wc = Wt.reshape(C, 3, 3, C).permute(0, 3, 1, 2).contiguous()        # [C_out, C_in, 3, 3]
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), Wc.double(), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(batch * g * g, C)
    assert float(ref.abs().max()) <= 128
    col = ops.im2col3(bf(x).reshape(-1, C).cuda(), batch, g)
    y = ops.linear(col, bf(Wt).cuda(), None, epilogue=EPI_BIAS)
    assert torch.equal(y.double().cpu(), ref)
