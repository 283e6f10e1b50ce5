"""GPU: the epilogue of the 8-phase GEMM (tile variant 31, csrc/gemm_8p_kernel.h) at the smallest shapes the variant takes.

The epilogue finishes a tile from the accumulator layout: the LayerNorm fold and the bias as two packed multiply-adds, the
activation in steps that are interleaved over two register pairs, one bf16 rounding, an exchange of one 16-byte block
between lanes r and r ^ 8 of every 16-lane row (a select and a move, both through DPP row_ror:8), and two 16-byte stores
per m-tile whose addresses are a wave-uniform part plus one lane term.  What can go wrong there is a value in the wrong
place or a step applied to the wrong register, and neither depends on the size of the problem, so:

  A  every activation (bias, erf-GELU, QuickGELU, tanh-GELU), with and without the fold: the bits of a ring4 variant on the
     same call (same products, same summation order, same epilogue formula) -- two rounds of tiles on every CU
  B  a ragged M over a padded A (NaN rows behind M): the bits of ring4, and the rows behind M of a larger output buffer
     keep the sentinel they were filled with
  C  both store policies: the plain stores of A (M N 2 bytes < 128 MB) and the non-temporal ones of an output above it
  D  designed operands: C[m, n] is a small integer, exact in bf16, that names the lane (m mod 16, (n / 8) mod 8) a value
     came from, and in a second pattern the m-tile and the 64-column wave (m / 16 mod 16, n / 64 mod 16), against plain
     torch fp32 -- an exchange that is routed wrongly in a self-consistent way cannot pass

Every entry point of the C ABI stores its output with a row stride of N, so an output with padding columns does not
exist at op level; the rows behind M of B are the memory next to the output that the kernel could reach.
"""
import pytest
import torch

from fixtures import ops  # noqa: F401
from ops_checks import bf

pytestmark = pytest.mark.gpu

K = 256
SENTINEL = 7.0


def _slots():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7  # one workgroup per CU, whole XCDs


def _rows(N):
    """two rounds of 256 x 256 tiles on every CU: the smallest M variant 31 takes at this N (gemm_8p_rounds)"""
    return 256 * (2 * _slots() // (N // 256))


def _epis():
    from vdr import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_TANH, EPI_BIAS_QUICK_GELU
    return {"bias": EPI_BIAS, "gelu": EPI_BIAS_GELU, "quick_gelu": EPI_BIAS_QUICK_GELU, "gelu_tanh": EPI_BIAS_GELU_TANH}


@pytest.fixture(scope="module")
def data(ops):
    """operands of A .. C, made once: x [M, K] with a quarter of the rows scaled into the clamped range of the erf form"""
    g = torch.Generator(device="cuda").manual_seed(8)
    M = _rows(512)
    x = torch.randn(M, K, generator=g, device="cuda")
    x[::4] *= 6.0
    d = dict(M=M, x=x.to(torch.bfloat16))
    for N in (512, 1024):
        d[N] = dict(W=(torch.randn(N, K, generator=g, device="cuda") * 0.06).to(torch.bfloat16),
                    b=torch.randn(N, generator=g, device="cuda"),
                    cs=torch.randn(N, generator=g, device="cuda"))
    st = torch.empty(M, 2, device="cuda")
    st[:, 0] = 0.2 * torch.randn(M, generator=g, device="cuda")
    st[:, 1] = 0.5 + torch.rand(M, generator=g, device="cuda")
    d["stats"] = st
    return d


def _call(ops, d, N, epi, fold, variant, M=None, out=None):
    w = d[N]
    M = d["M"] if M is None else M
    if fold:
        return ops.linear_ln_fold(d["x"], w["W"], w["cs"], w["b"], variant, epilogue=epi, stats=d["stats"], M=M, out=out)
    assert M == d["M"]
    packed = variant >= 26 and variant != 31
    return ops.linear(d["x"], ops.pack_linear_weight(w["W"]) if packed else w["W"], w["b"], epilogue=epi, variant=variant,
                      packed=packed, out=out)


# ---- A ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("kind", ["bias", "gelu", "quick_gelu", "gelu_tanh"])
def test_every_activation_is_ring4_bit_for_bit(ops, data, kind, fold):
    epi = _epis()[kind]
    assert data["M"] * 512 * 2 < 128e6  # the plain store policy
    y = _call(ops, data, 512, epi, fold, 31)
    ref = _call(ops, data, 512, epi, fold, 26)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), (kind, fold)


# ---- B ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bias", "gelu"])
def test_ragged_m_over_padded_a(ops, data, kind):
    epi = _epis()[kind]
    Mr = data["M"]
    M = Mr - 100  # the last tile row holds 156 rows: its second M half 28, one m-tile cut inside
    d = dict(data)
    d["x"] = data["x"].clone()
    d["x"][M:] = float("nan")  # readable padding: multiplied, never stored
    d["stats"] = data["stats"].clone()
    d["stats"][M:] = float("nan")
    out = torch.full((Mr + 256, 512), SENTINEL, dtype=torch.bfloat16, device="cuda")
    _call(ops, d, 512, epi, True, 31, M=M, out=out)
    ref = _call(ops, d, 512, epi, True, 26, M=M)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(out[:M].view(torch.int16), ref.view(torch.int16)), kind
    assert (out[M:] == SENTINEL).all(), "rows behind M were written"


# ---- C ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
def test_non_temporal_store_policy(ops, data, fold):
    from vdr import EPI_BIAS_GELU
    assert data["M"] * 1024 * 2 >= 128e6  # above the switch (csrc/gemm_launch.h output_exceeds_cache)
    y = _call(ops, data, 1024, EPI_BIAS_GELU, fold, 31)
    ref = _call(ops, data, 1024, EPI_BIAS_GELU, fold, 26)
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), fold


# ---- D ----------------------------------------------------------------------------------------------------------
def _designed(M, N, row_code, col_code):
    """A, W with C[m, n] = row_code(m) + col_code(n): A[m, row_code(m)] = 1 and A[m, 16] = 1; W[n, k] = k for k < 16,
    W[n, 16] = col_code(n).  Every product and sum is a small integer."""
    m = torch.arange(M)
    n = torch.arange(N)
    A = torch.zeros(M, K)
    A[m, row_code(m)] = 1.0
    A[:, 16] = 1.0
    W = torch.zeros(N, K)
    W[:, :16] = torch.arange(16.0)
    W[:, 16] = col_code(n).float()
    return A, W


@pytest.mark.parametrize("N", [512, 1024])  # plain and non-temporal stores
@pytest.mark.parametrize("pattern", ["lane", "tile"])
def test_designed_integers_name_their_origin(ops, N, pattern):
    from vdr import EPI_BIAS
    Mr = _rows(512)
    M = Mr - 100
    if pattern == "lane":  # the lane of the accumulator layout: row r of a 16-row m-tile, 8-column group of a 64-column block
        A, W = _designed(Mr, N, lambda m: m % 16, lambda n: 16 * ((n // 8) % 8))
    else:                  # the m-tile of the 256-row tile, the wave's 64 columns and the tile column
        A, W = _designed(Mr, N, lambda m: (m // 16) % 16, lambda n: 16 * ((n // 64) % 16))
    ref = A @ W.t()  # plain torch fp32
    assert ref.max() <= 255 and torch.equal(ref, bf(ref).float())
    x, Wd = bf(A).cuda(), bf(W).cuda()
    ref = ref.cuda()
    # without the fold: whole tiles
    y = ops.linear(x, Wd, None, epilogue=EPI_BIAS, variant=31)
    assert torch.equal(y.float(), ref), (pattern, N)
    # with it, (mean, rstd) = (0, 1): rs acc + (-0 colsum + 0) is acc exactly; ragged M into a larger buffer
    st = torch.zeros(Mr, 2, device="cuda")
    st[:, 1] = 1.0
    cs = torch.arange(N, device="cuda").float()
    out = torch.full((Mr + 256, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ops.linear_ln_fold(x, Wd, cs, torch.zeros(N, device="cuda"), 31, epilogue=EPI_BIAS, stats=st, M=M, out=out)
    assert torch.equal(out[:M].float(), ref[:M]), (pattern, N, "ragged")
    assert (out[M:] == SENTINEL).all(), "rows behind M were written"
