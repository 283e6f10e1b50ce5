"""GPU: vdr_op_log_bin (csrc/log_bin.hip) at op level against the brute-force restatement of its definition
(tests/descriptor_ref.py log_bin_brute: window sums exact in float64, one fp32 division by the in-grid count).

Designed inputs are integer-valued bf16 with |v| <= 64: every fp32 window sum (at most 81 terms, |sum| <= 5184 < 2^24) is
exact in any order, so the fp32 output must equal the restatement bit for bit and the bf16 output its single rounding.
Grids: 1x1, 2x3 (every neighbour clamped), 7x5, 10x11 (a 9-wide window that touches both edges); C = 8 (one 16-byte
chunk), 72 (9 chunks, not a multiple of the 64 lanes of a wave), 384 (a real width, more than one pass of a workgroup
over an output row); batch 1 and 3."""
import numpy as np
import pytest
import torch

import descriptor_ref as dref
from fixtures import ops  # noqa: F401

pytestmark = pytest.mark.gpu

GRIDS = ((1, 1), (2, 3), (7, 5), (10, 11))
HIERARCHIES = (1, 2, 3)
WIDTHS = (8, 72, 384)


_CACHE = {}


def _designed(gh, gw, Cc):
    """(x [3, n, C] integer-valued fp32, {h: restatement (a) of it}) -- computed once per shape, shared, never written"""
    key = (gh, gw, Cc)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1000 * gh + 100 * gw + Cc)
        x = torch.randint(-64, 65, (3, gh * gw, Cc), generator=gen).float()
        _CACHE[key] = (x, {h: torch.from_numpy(dref.log_bin_brute(x, gh, gw, h)) for h in HIERARCHIES})
    return _CACHE[key]


@pytest.mark.parametrize("h", HIERARCHIES)
@pytest.mark.parametrize("grid", GRIDS)
def test_designed_inputs_are_exact(ops, grid, h):
    gh, gw = grid
    for Cc in WIDTHS:
        x, refs = _designed(gh, gw, Cc)
        ref = refs[h]
        for B in (1, 3):
            xb = x[:B].to(torch.bfloat16).cuda()
            got = ops.log_bin(xb, gh, gw, h, torch.float32).cpu()
            assert got.shape == (B, gh * gw, (1 + 8 * h) * Cc)
            assert torch.equal(got, ref[:B]), (grid, h, Cc, B, float((got - ref[:B]).abs().max()))
            g16 = ops.log_bin(xb, gh, gw, h, torch.bfloat16).cpu()
            assert g16.dtype == torch.bfloat16 and torch.equal(g16, ref[:B].to(torch.bfloat16)), (grid, h, Cc, B)
        # fp32 source rows (the residual stream's fp32 master copy): the same values, the same bits
        x32 = x.cuda()
        assert torch.equal(ops.log_bin(x32, gh, gw, h, torch.float32).cpu(), ref), (grid, h, Cc)
        assert torch.equal(ops.log_bin(x32, gh, gw, h, torch.bfloat16).cpu(), ref.to(torch.bfloat16)), (grid, h, Cc)


@pytest.mark.parametrize("P", (1, 5))
@pytest.mark.parametrize("grid", GRIDS)
def test_strided_source_in_place_and_sentinels(ops, grid, P):
    """The same data as the key columns and patch rows of a [B, P + n, 3C] qkv-like buffer (ld = 3C, column offset C):
    bits equal the contiguous run, for both dtypes; rows in front of and behind `out` are untouched."""
    gh, gw = grid
    n = gh * gw
    for Cc in WIDTHS:
        x, _ = _designed(gh, gw, Cc)
        xb = x.to(torch.bfloat16)
        gen = torch.Generator().manual_seed(5)
        buf = torch.randint(-64, 65, (3, P + n, 3 * Cc), generator=gen).to(torch.bfloat16)
        buf[:, P:, Cc:2 * Cc] = xb
        buf = buf.cuda()
        view = buf[:, P:, Cc:2 * Cc]
        assert not view.is_contiguous() or n == 1
        for h in HIERARCHIES:
            for dt in (torch.float32, torch.bfloat16):
                want = ops.log_bin(xb.cuda(), gh, gw, h, dt)
                W = (1 + 8 * h) * Cc
                big = torch.full((3 * n + 2, W), -7.0, dtype=dt, device="cuda")
                out = big[1:-1].view(3, n, W)
                ops.log_bin(view, gh, gw, h, dt, out=out)
                assert torch.equal(out, want), (grid, P, Cc, h, dt)
                assert torch.all(big[0] == -7.0) and torch.all(big[-1] == -7.0), (grid, P, Cc, h, dt)


@pytest.mark.parametrize("h", HIERARCHIES)
@pytest.mark.parametrize("grid", GRIDS)
def test_random_inputs_within_the_summation_bound(ops, grid, h):
    """Random bf16 input, fp32 output: |got - ref(a)| <= 2 (9^(h-1) - 1) 2^-24 max|x| + one ulp of the value -- the fp32
    summation-order bound of a window of 9^(h-1) terms, taken twice (reference and kernel may each use any order), plus the
    division's rounding.  Level-0 bins are bitwise copies."""
    gh, gw = grid
    Cc = 72
    gen = torch.Generator().manual_seed(31 + 100 * gh + 10 * gw + h)
    x = (torch.randn(2, gh * gw, Cc, generator=gen) * 3).to(torch.bfloat16)
    ref = dref.log_bin_brute(x.float(), gh, gw, h)
    got = ops.log_bin(x.cuda(), gh, gw, h, torch.float32).cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = dref.log_bin_bound(x, h, ref)
    print(f"log_bin {gh}x{gw} h={h}: max err {err.max():.3e}, min slack {(bound - err).min():.3e}")
    assert (err <= bound).all(), (grid, h, float(err.max()))
    assert np.array_equal(got[:, :, :9 * Cc], ref[:, :, :9 * Cc])


@pytest.mark.parametrize("h", HIERARCHIES)
def test_an_image_has_the_same_bits_at_any_batch_position(ops, h):
    gh, gw, Cc = 7, 5, 72
    gen = torch.Generator().manual_seed(77 + h)
    x = torch.randn(3, gh * gw, Cc, generator=gen).to(torch.bfloat16)
    x[2] = x[0]
    for dt in (torch.float32, torch.bfloat16):
        three = ops.log_bin(x.cuda(), gh, gw, h, dt)
        one = ops.log_bin(x[:1].cuda(), gh, gw, h, dt)
        assert torch.equal(three[2], one[0]) and torch.equal(three[0], one[0]), (h, dt)


def test_refusals_leave_the_output_alone():
    from vdr import _lib
    lib = _lib.load()
    BF, F32 = _lib.VDR_BF16, _lib.VDR_F32
    gh, gw, Cc = 2, 3, 16
    x = torch.ones(1, gh * gw, Cc, dtype=torch.bfloat16, device="cuda")
    work = torch.zeros(2 * gh * gw * Cc, dtype=torch.float32, device="cuda")
    out = torch.full((gh * gw * 25 * Cc + 8,), -3.0, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(x=x.data_ptr(), in_dtype=BF, ld=Cc, image_stride=gh * gw * Cc, batch=1, gh=gh, gw=gw, Cc=Cc, h=2, work=work.data_ptr(),
             out=out.data_ptr(), out_dtype=F32):
        return lib.vdr_op_log_bin(x, in_dtype, ld, image_stride, batch, gh, gw, Cc, h, work, out, out_dtype, s)

    for h in (0, 4, -1):
        assert call(h=h) == -7, h  # VDR_ERR_UNSUPPORTED
    invalid = [dict(Cc=12, ld=12), dict(Cc=4, ld=4), dict(ld=Cc - 8), dict(x=None), dict(out=None), dict(work=None), dict(batch=0),
               dict(gh=0), dict(gw=0), dict(Cc=0), dict(x=x.data_ptr() + 2), dict(x=x.data_ptr() + 8), dict(out=out.data_ptr() + 4),
               dict(work=work.data_ptr() + 8), dict(ld=Cc + 4), dict(image_stride=gh * gw * Cc + 4), dict(in_dtype=2), dict(out_dtype=3)]
    for kw in invalid:
        assert call(**kw) == -1, kw  # VDR_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(out == -3.0)
    # ... and the well-formed call writes exactly its [1, n, 17 C] elements
    assert call() == 0
    torch.cuda.synchronize()
    nout = gh * gw * 17 * Cc
    assert torch.all(out[:nout] == 1.0) and torch.all(out[nout:] == -3.0)


def test_ops_log_bin_checks_a_caller_owned_out(ops):
    """A wrong out tensor is a ValueError on the host, never an out-of-bounds device write."""
    gh, gw, Cc = 2, 3, 16
    x = torch.ones(2, gh * gw, Cc, dtype=torch.bfloat16, device="cuda")
    good = torch.empty(2, gh * gw, 17 * Cc, device="cuda")
    assert ops.log_bin(x, gh, gw, 2, out=good) is good and torch.all(good == 1.0)
    bad = [torch.empty(2, gh * gw, 9 * Cc, device="cuda"), torch.empty(1, gh * gw, 17 * Cc, device="cuda"),
           torch.empty(2, gh * gw, 17 * Cc), torch.empty(2, gh * gw, 17 * Cc, dtype=torch.float16, device="cuda"),
           torch.empty(2, gh * gw, 34 * Cc, device="cuda")[:, :, ::2]]
    for out in bad:
        with pytest.raises(ValueError, match="out must be"):
            ops.log_bin(x, gh, gw, 2, out=out)
    for h in (0, 4):
        with pytest.raises(ValueError, match="hierarchy"):
            ops.log_bin(x, gh, gw, h)
