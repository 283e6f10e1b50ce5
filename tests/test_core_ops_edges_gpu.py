"""GPU: vdr_op_linear / vdr_op_linear_packed and vdr_op_layernorm at their smallest shapes, inside guards.

The forward runs GEMMs of a handful of rows (the CLS tail, classifier heads) and LayerNorms of any width D % 4 == 0, into
caller-owned views; the older operator tests launch nothing below 64 x 64 x 64 or D = 192, always into fresh allocations.
Here every launch has
  * its inputs as slices out of the middle of NaN-filled allocations (a read outside the operand shows as a NaN),
  * its output in the middle of a canary-filled allocation with guard rows on both sides (a write outside shows in the
    guards, a missing write as a canary left in the body),
and must give the bits of the same launch on fresh, separate allocations.  Exactness comes from designed inputs
(tests/core_ops_designs.py): integer data for BIAS / RESID, the +32 / -128 gate design for SwiGLU, saturated
pre-activations for the three GELU forms; LayerNorm is gated by a bound derived from its arithmetic (ln_bound), against a
float64 LayerNorm, never against the kernel.

SwiGLU exactness rests on v_rcp_f32(1.0) == 1.0; the MI355X returned exactly that ("Core operators at their
edges").
"""
import pytest
import torch

import core_ops_designs as cd
import memguard as mg
from fixtures import ops  # noqa: F401
from ops_checks import BF16_EPS, bf

pytestmark = pytest.mark.gpu

VARIANTS = [22, 23, 24, 25, 26, 27, 28, 29]
# one row; fewer rows than any wave tile; a ragged last tile in M and in N for the 64-, 128- and 256-wide tiles
SHAPES = [(1, 8, 64), (7, 72, 64), (65, 136, 128), (129, 264, 192), (257, 520, 64)]
SWIGLU_SHAPES = [(1, 64, 64), (7, 128, 64), (129, 320, 128), (257, 576, 192)]
GUARD_ROWS = 8
DT_PAIRS = [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16),
            (torch.float32, torch.float32)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Linear:
    """One linear launch described on the host (fp32 tensors holding bf16-exact x / W / resid), run either on fresh
    allocations or inside NaN surroundings and guard rows."""

    def __init__(self, ops, x, W, bias, epi, variant, packed, resid=None, gamma=None, inplace=False):
        self.ops, self.epi, self.variant, self.packed, self.inplace = ops, epi, variant, packed, inplace
        self.x, self.W, self.bias, self.resid, self.gamma = bf(x), bf(W), bias, None if resid is None else bf(resid), gamma
        from vdr import EPI_SWIGLU
        self.n_out = W.shape[0] // 2 if epi == EPI_SWIGLU else W.shape[0]

    def _weight(self):
        Wd = self.W.cuda()
        return self.ops.pack_linear_weight(Wd) if self.packed else Wd

    def fresh(self):
        opt = lambda t: None if t is None else t.cuda()  # noqa: E731
        r = opt(self.resid)
        out = r if self.inplace else None
        return self.ops.linear(self.x.cuda(), self._weight(), opt(self.bias), resid=r, gamma=opt(self.gamma), epilogue=self.epi,
                               variant=self.variant, packed=self.packed, out=out)

    def guarded(self):
        """the output body (a copy), after asserting guard rows intact and no canary left in the body"""
        M = self.x.shape[0]
        nan = lambda t: None if t is None else mg.inside_nan(t, GUARD_ROWS)  # noqa: E731  (8 rows / 8 floats: 16-byte steps)
        whole, body = mg.guarded_rows(M, self.n_out, torch.bfloat16, GUARD_ROWS)
        r = nan(self.resid)
        if self.inplace:
            body.copy_(self.resid)
            r = body
        Wd = mg.inside_nan(self._weight().cpu(), GUARD_ROWS)  # (a packed weight is an opaque [N, K] bf16 tensor: copied bit for bit)
        for t in (r, Wd):
            assert t is None or t.data_ptr() % 16 == 0
        self.ops.linear(nan(self.x), Wd, nan(self.bias), resid=r, gamma=nan(self.gamma), epilogue=self.epi, variant=self.variant,
                        packed=self.packed, out=body)
        torch.cuda.synchronize()
        what = (tuple(self.x.shape), self.W.shape[0], self.epi, self.variant, self.packed, self.inplace)
        assert mg.rows_intact(whole, GUARD_ROWS), f"guard rows overwritten {what}"
        assert mg.canary_left(body) == 0, f"{mg.canary_left(body)} output elements never written {what}"
        return body.clone()


def _close(got, ref, atol, what):
    got, ref = got.float().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), what
    bad = (got - ref).abs() > atol + BF16_EPS * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} outside tolerance, max err {(got - ref).abs().max():.4g}"


def _random_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(M, K, generator=g)).float()
    W = bf(torch.randn(N, K, generator=g) * 0.08).float()
    b = torch.randn(N, generator=g) * 0.1
    r = bf(torch.randn(M, N, generator=g)).float()
    gamma = 1 + 0.2 * torch.randn(N, generator=g)
    return x, W, b, r, gamma


# ---- linear ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_linear_every_epilogue_small_shapes_inside_guards(ops, variant, packed):
    """Every public epilogue on random data: guard rows intact, every output element written, the bits of the same launch
    on fresh allocations, and the values within one bf16 rounding (+ the summation noise the older tests allow: 3e-3
    sqrt(K / 768) absolute) of a float64 reference."""
    import vdr
    for (M, N, K) in SHAPES:
        x, W, b, r, gamma = _random_case(M, N, K, 1000 * variant + M)
        lin = x.double() @ W.double().t() + b.double()
        cases = [
            ("bias", vdr.EPI_BIAS, {}, lin),
            ("gelu", vdr.EPI_BIAS_GELU, {}, torch.nn.functional.gelu(lin)),
            ("quick_gelu", vdr.EPI_BIAS_QUICK_GELU, {}, lin * torch.sigmoid(1.702 * lin)),
            ("gelu_tanh", vdr.EPI_BIAS_GELU_TANH, {}, torch.nn.functional.gelu(lin, approximate="tanh")),
            ("resid", vdr.EPI_BIAS_RESID, dict(resid=r), r.double() + lin),
            ("resid_gamma", vdr.EPI_BIAS_RESID, dict(resid=r, gamma=gamma), r.double() + gamma.double() * lin),
            ("resid_inplace", vdr.EPI_BIAS_RESID, dict(resid=r, inplace=True), r.double() + lin),
            ("resid_gamma_inplace", vdr.EPI_BIAS_RESID, dict(resid=r, gamma=gamma, inplace=True), r.double() + gamma.double() * lin),
        ]
        for name, epi, kw, ref in cases:
            L = Linear(ops, x, W, b, epi, variant, packed, **kw)
            got = L.guarded()
            assert torch.equal(_bits(got), _bits(L.fresh())), (name, M, N, K)
            _close(got, ref, 3e-3 * (K / 768) ** 0.5 + 1e-6, f"{name} {(M, N, K)} variant {variant}")
    for (M, N, K) in SWIGLU_SHAPES:
        x, w12, b12, _, _ = _random_case(M, N, K, 2000 * variant + M)
        pre = x.double() @ w12.double().t() + b12.double()
        a, u = pre.chunk(2, dim=-1)
        wp, bp = ops.pack_w12(w12, b12)
        L = Linear(ops, x, wp, bp, vdr.EPI_SWIGLU, variant, packed)
        got = L.guarded()
        assert got.shape == (M, N // 2)
        assert torch.equal(_bits(got), _bits(L.fresh())), ("swiglu", M, N, K)
        _close(got, torch.nn.functional.silu(a) * u, 2e-3, f"swiglu {(M, N, K)} variant {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_linear_small_shapes_integer_exact_and_packed_equals_plain(ops, variant):
    """BIAS and RESID on integer data (every product and partial sum exact in fp32, |y| <= 256 exact in bf16): the bits of
    the fp32 reference, inside guards, for the plain and the packed weight -- whose bits are therefore equal (vdr.h's
    promise); on random data, where nothing is exact, the packed launch equals the plain one bit for bit as well."""
    import vdr
    g = torch.Generator().manual_seed(variant)
    for (M, N, K) in SHAPES:
        x = torch.randint(-2, 3, (M, K), generator=g).float()
        W = torch.randint(-2, 3, (N, K), generator=g).float()
        b = torch.randint(-3, 4, (N,), generator=g).float()
        r = torch.randint(-4, 5, (M, N), generator=g).float()
        ref = x @ W.t() + b
        assert (ref + r).abs().max() <= 256
        for packed in (False, True):
            y = Linear(ops, x, W, b, vdr.EPI_BIAS, variant, packed).guarded()
            assert torch.equal(y.float().cpu(), ref), (variant, packed, "bias", M, N, K)
            for inplace in (False, True):
                y = Linear(ops, x, W, b, vdr.EPI_BIAS_RESID, variant, packed, resid=r, inplace=inplace).guarded()
                assert torch.equal(y.float().cpu(), ref + r), (variant, packed, "resid", inplace, M, N, K)
        xr, Wr, br, rr, gr = _random_case(M, N, K, 77 * variant + N)
        for epi, kw in ((vdr.EPI_BIAS, {}), (vdr.EPI_BIAS_GELU, {}), (vdr.EPI_BIAS_RESID, dict(resid=rr, gamma=gr))):
            plain = Linear(ops, xr, Wr, br, epi, variant, False, **kw).guarded()
            assert torch.equal(_bits(plain), _bits(Linear(ops, xr, Wr, br, epi, variant, True, **kw).guarded())), (variant, epi, M, N, K)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_linear_bias_is_local_in_rows_and_columns(ops, variant, packed):
    """One NaN in row i of x makes exactly row i of y NaN, one NaN in row j of W exactly column j; every other bit stays."""
    import vdr
    for (M, N, K) in SHAPES:
        x, W, b, _, _ = _random_case(M, N, K, 31 * variant + K)
        base = Linear(ops, x, W, b, vdr.EPI_BIAS, variant, packed).guarded()
        assert torch.isfinite(base.float()).all()
        for i in sorted({0, M // 2, M - 1}):
            xn = x.clone()
            xn[i, (7 * i + 3) % K] = float("nan")
            y = Linear(ops, xn, W, b, vdr.EPI_BIAS, variant, packed).guarded()
            keep = torch.ones(M, dtype=torch.bool, device=y.device)
            keep[i] = False
            assert torch.isnan(y[i].float()).all(), (variant, packed, "x row", i, M, N, K)
            assert torch.equal(_bits(y[keep]), _bits(base[keep])), (variant, packed, "x row", i, M, N, K)
        for j in sorted({0, N // 2, N - 1}):
            Wn = W.clone()
            Wn[j, (5 * j + 1) % K] = float("nan")
            y = Linear(ops, x, Wn, b, vdr.EPI_BIAS, variant, packed).guarded()
            keep = torch.ones(N, dtype=torch.bool, device=y.device)
            keep[j] = False
            assert torch.isnan(y[:, j].float()).all(), (variant, packed, "W row", j, M, N, K)
            assert torch.equal(_bits(y[:, keep]), _bits(base[:, keep])), (variant, packed, "W row", j, M, N, K)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_swiglu_designed_gates_exact(ops, variant, packed):
    """The +32 / -128 gate design: every output is 32 u or a signed zero, so a swapped gate / value half, a pairing off by
    one 32-block, a wrong output column or a dropped bias half changes bits (shown on the CPU for each).  Compared bit for
    bit, zeros' signs included, with the fp32 restatement of the epilogue."""
    import vdr
    for (M, N, K) in SWIGLU_SHAPES:
        x, W, b, bit = cd.swiglu_design(M, N, K)
        want = cd.swiglu_eval(x, W, b)
        assert torch.equal(want.float(), cd.swiglu_expected(x, W, b, bit))
        got = Linear(ops, x, W, b, vdr.EPI_SWIGLU, variant, packed).guarded().cpu()
        diff = _bits(got) != _bits(want)
        if diff.any():
            i = torch.nonzero(diff)[0].tolist()
            raise AssertionError(f"swiglu design {(M, N, K)} variant {variant} packed {packed}: {int(diff.sum())} elements differ, first "
                                 f"at {i}: got {got[tuple(i)].item()} want {want[tuple(i)].item()}")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_saturated_gelu_forms_return_their_integer(ops, variant, packed):
    """Pre-activations that are integers in [8, 199], coding row and column: each of the three GELU epilogues returns the
    integer itself after the bf16 rounding (core_ops_designs.GELU_RANGE, checked on the CPU for every integer)."""
    import vdr
    for (M, N, K) in SHAPES:
        x, W, b, want = cd.gelu_design(M, N, K)
        for epi in (vdr.EPI_BIAS_GELU, vdr.EPI_BIAS_QUICK_GELU, vdr.EPI_BIAS_GELU_TANH):
            got = Linear(ops, x, W, b, epi, variant, packed).guarded()
            assert torch.equal(got.float().cpu(), want), (variant, packed, epi, M, N, K)


def test_rcp_of_one_is_one(ops):
    """The one hardware fact the SwiGLU design rests on, measured: silu(+32) = 32 * rcp(1 + 2^-46) must be exactly 32."""
    import vdr
    K = 64
    x = torch.zeros(4, K)
    W = torch.zeros(64, K)
    b = torch.cat([torch.full((32,), 32.0), torch.ones(32)])
    y = ops.linear(bf(x).cuda(), bf(W).cuda(), b.cuda(), epilogue=vdr.EPI_SWIGLU)
    print("silu(32) * 1 on the device:", y[0, 0].item())
    assert torch.equal(y.float().cpu(), torch.full((4, 32), 32.0))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
def _ln_guarded(ops, x, gamma, beta, eps, out_dt, pad=GUARD_ROWS):
    whole, body = mg.guarded_rows(x.shape[0], x.shape[1], out_dt, GUARD_ROWS)
    ops.layernorm(mg.inside_nan(x, pad), mg.inside_nan(gamma, 8), mg.inside_nan(beta, 8), eps, out_dt, out=body)
    torch.cuda.synchronize()
    assert mg.rows_intact(whole, GUARD_ROWS), ("guard rows overwritten", tuple(x.shape), x.dtype, out_dt)
    assert mg.canary_left(body) == 0, ("output elements never written", tuple(x.shape), x.dtype, out_dt)
    return body.clone()


@pytest.mark.parametrize("in_dt,out_dt", DT_PAIRS)
def test_layernorm_every_width_class_inside_guards(ops, in_dt, out_dt):
    """D from one vector (4) to the limit (2048), on both sides of every 256-column pass boundary, with 1 .. 9 rows (the
    workgroup takes 4): guards, canary, the bits of a fresh launch (ops.layernorm's default path), locality of a NaN row,
    and accuracy against a float64 LayerNorm inside core_ops_designs.ln_bound -- derived from the kernel's arithmetic
    (two-pass fp32 statistics, rsqrtf, one affine, one rounding), gate: error / bound <= 1 for every element."""
    worst = 0.0
    for D in cd.LN_WIDTHS:
        for rows in cd.LN_ROWS:
            x, gamma, beta = cd.ln_inputs(D, rows, in_dt)
            for eps in (1e-6, 1e-5):
                got = _ln_guarded(ops, x, gamma, beta, eps, out_dt)
                fresh = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), eps, out_dt)
                assert fresh.dtype == out_dt and torch.equal(_bits(got), _bits(fresh)), (D, rows, eps)
                r = cd.worst_ratio(got.cpu(), x, gamma, beta, eps, out_dt)
                worst = max(worst, r)
                assert r <= 1.0, f"LayerNorm D={D} rows={rows} eps={eps} {in_dt}->{out_dt}: error / bound = {r:.3f}"
            if rows > 1:
                i = rows // 2
                xn = x.clone()
                xn[i, D - 1] = float("nan")
                y = _ln_guarded(ops, xn, gamma, beta, 1e-5, out_dt)
                keep = torch.ones(rows, dtype=torch.bool, device=y.device)
                keep[i] = False
                assert torch.isnan(y[i].float()).all(), (D, rows)
                assert torch.equal(_bits(y[keep]), _bits(got[keep])), (D, rows)
    print(f"LayerNorm {in_dt} -> {out_dt}: worst error / bound = {worst:.3f}")


def test_layernorm_offset_rows_keep_the_bound(ops):
    """fp32 rows of 1000 + N(0, 1) at D = 1024: inside the same bound only while the variance is two-pass (an fp32
    E[x^2] - mean^2 exceeds it 100-fold for this seed: tests/test_core_ops_designs_cpu.py)."""
    x, gamma, beta = cd.ln_offset_case()
    for out_dt in (torch.float32, torch.bfloat16):
        got = _ln_guarded(ops, x, gamma, beta, 1e-6, out_dt)
        r = cd.worst_ratio(got.cpu(), x, gamma, beta, 1e-6, out_dt)
        print(f"LayerNorm offset rows fp32 -> {out_dt}: worst error / bound = {r:.3f}")
        assert r <= 1.0


def _raw_layernorm(x, y, gamma, beta, rows, D, in_dt=torch.float32, out_dt=torch.float32):
    from vdr import _lib as L
    code = lambda dt: 1 if dt == torch.bfloat16 else 0  # noqa: E731
    L.check(L.load().vdr_op_layernorm(x.data_ptr(), code(in_dt), y.data_ptr(), code(out_dt), gamma.data_ptr(), beta.data_ptr(),
                                      rows, D, 1e-6, torch.cuda.current_stream().cuda_stream))


def _untouched(buf):
    torch.cuda.synchronize()
    return bool((buf.view(torch.uint8) == mg.CANARY).all())


def test_layernorm_refusals_leave_the_output_alone(ops):
    import vdr
    x = torch.zeros(4 * 2052, device="cuda")
    gamma = torch.ones(2052, device="cuda")
    y = torch.full((4 * 2052 * 4,), mg.CANARY, dtype=torch.uint8, device="cuda")
    for rows, D in ((4, 6), (4, 2), (4, 2052), (4, 0), (0, 64), (-1, 64), (4, -4)):
        with pytest.raises(vdr.VdrError):
            _raw_layernorm(x, y, gamma, gamma, rows, D)
        assert _untouched(y), (rows, D)
    _raw_layernorm(x, y, gamma, gamma, 4, 2048)  # (the same buffers, a shape inside the limits: accepted)
    assert not _untouched(y)


def test_misaligned_pointers_are_refused_before_any_launch(ops):
    """x, W, bias, resid, gamma, y of the linears on 16 bytes; LayerNorm's x / y on 4 elements (8 bytes of bf16, 16 of fp32),
    gamma / beta on 16 bytes.  Each pointer in turn is a slice that starts off that boundary: VDR_ERR_INVALID, and the
    canary-filled output keeps every byte (nothing is launched on a misaligned pointer)."""
    import vdr
    from vdr import _lib as L
    M, N, K = 8, 16, 64
    buf = lambda n, dt: torch.zeros(n + 16, dtype=dt, device="cuda")  # noqa: E731
    xs, Ws, rs = buf(M * K, torch.bfloat16), buf(N * K, torch.bfloat16), buf(M * N, torch.bfloat16)
    bs, gs = buf(N, torch.float32), buf(N, torch.float32)
    ys = torch.full(((M * N + 16) * 2,), mg.CANARY, dtype=torch.uint8, device="cuda").view(torch.bfloat16)
    names = ("x", "W", "bias", "resid", "gamma", "y")
    for packed in (False, True):
        for bad in names:
            for off_bytes in (2, 4, 8):
                def cut(t, name, n, shape):
                    o = off_bytes // t.dtype.itemsize if name == bad else 0
                    if name == bad and o == 0:
                        o = 1  # (fp32: the smallest step off the boundary is 4 bytes)
                    return t[o:o + n].view(shape)
                x, W = cut(xs, "x", M * K, (M, K)), cut(Ws, "W", N * K, (N, K))
                r, y = cut(rs, "resid", M * N, (M, N)), cut(ys, "y", M * N, (M, N))
                b, g = cut(bs, "bias", N, (N,)), cut(gs, "gamma", N, (N,))
                with pytest.raises(vdr.VdrError) as e:
                    ops.linear(x, W, b, resid=r, gamma=g, epilogue=vdr.EPI_BIAS_RESID, variant=22, out=y, packed=packed)
                assert e.value.code == -1, (bad, off_bytes, e.value)  # VDR_ERR_INVALID
                assert _untouched(ys), (bad, off_bytes)
    ops.linear(xs[:M * K].view(M, K), Ws[:N * K].view(N, K), bs[:N], resid=rs[:M * N].view(M, N), gamma=gs[:N],
               epilogue=vdr.EPI_BIAS_RESID, variant=22, out=ys[:M * N].view(M, N))  # (aligned: accepted)
    assert not _untouched(ys)
    # LayerNorm
    rows, D = 4, 64
    for in_dt, out_dt in DT_PAIRS:
        xb, gb, bb = buf(rows * D, in_dt), buf(D, torch.float32), buf(D, torch.float32)
        yb = torch.full(((rows * D + 16) * out_dt.itemsize,), mg.CANARY, dtype=torch.uint8, device="cuda").view(out_dt)
        dts = {"x": in_dt, "y": out_dt, "gamma": torch.float32, "beta": torch.float32}
        for bad in ("x", "y", "gamma", "beta"):
            # element offsets off the boundary: fp32 needs 16 bytes (1, 2, 3 elements are off), bf16 x / y 8 bytes (1, 3)
            for o in (1, 2, 3) if dts[bad] == torch.float32 else (1, 3):
                off = {k: (o if k == bad else 0) for k in ("x", "y", "gamma", "beta")}
                with pytest.raises(vdr.VdrError) as e:
                    _raw_layernorm(xb[off["x"]:], yb[off["y"]:], gb[off["gamma"]:], bb[off["beta"]:], rows, D, in_dt, out_dt)
                assert e.value.code == -1, (bad, o, e.value)
                assert _untouched(yb), (bad, o)
        if in_dt == torch.bfloat16 and out_dt == torch.bfloat16:  # 8 bytes is enough for bf16 rows: accepted
            _raw_layernorm(xb[4:], yb[4:], gb, bb, rows, D, in_dt, out_dt)
            torch.cuda.synchronize()
            assert bool((yb[:4].view(torch.uint8) == mg.CANARY).all()) and mg.canary_left(yb[4:4 + rows * D]) == 0
    assert L.load().vdr_last_error(None)  # the refusals left their text


def test_attention_entry_points_refuse_non_positive_shapes(ops):
    """vdr_op_attention, _hd and _varlen: batch, seq, heads <= 0 are VDR_ERR_INVALID at the entry point; the canary-filled
    output keeps every byte."""
    import vdr
    from vdr import _lib as L
    lib = L.load()
    B, S, H, dh = 2, 8, 2, 64
    qkv = torch.zeros(B * S, 3 * H * dh, dtype=torch.bfloat16, device="cuda")
    out = torch.full((B * S * H * dh * 2,), mg.CANARY, dtype=torch.uint8, device="cuda")
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for b, n, h in ((0, S, H), (B, 0, H), (B, S, 0), (-1, S, H), (B, -3, H), (B, S, -2)):
        for call in (lambda: lib.vdr_op_attention(qkv.data_ptr(), out.data_ptr(), b, n, h, 0, s),
                     lambda: lib.vdr_op_attention_hd(qkv.data_ptr(), out.data_ptr(), b, n, h, dh, 0, s),
                     lambda: lib.vdr_op_attention_varlen(qkv.data_ptr(), out.data_ptr(), b, n, h, dh, lens.data_ptr(), 0, 0, s)):
            with pytest.raises(vdr.VdrError) as e:
                L.check(call())
            assert e.value.code == -1, (b, n, h, e.value)
            assert _untouched(out), (b, n, h)
    got = ops.attention(qkv, B, S, H)  # (the same operand at its real shape: accepted)
    assert got.shape == (B * S, H * dh) and torch.isfinite(got.float()).all()
