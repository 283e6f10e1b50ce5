"""Plain-torch reference pieces shared by tests/test_sam_ops_cpu.py and tests/test_sam_ops_gpu.py: the row maps of
segment_anything's window_partition / window_unpartition, the byte offsets of an MX tensor's scales and the designed
inputs of the SAM op tests.  tests/test_sam_ops_cpu.py proves the row maps against oracle.sam_oracle, so the GPU tests
stand on a checked reference and not on a restatement of the kernels' index arithmetic."""
import torch

# (batch, g, ws): the smallest geometries at which the window path can go wrong
GEOMETRIES = [
    (3, 10, 4),    # padded, nw = 3
    (2, 14, 7),    # no padding
    (2, 14, 4),    # padded
    (2, 3, 7),     # g < ws: one partly filled window
    (5, 13, 14),   # g < ws, 196-row windows
    (2, 15, 14),   # g = ws + 1: border windows with one valid row or column
    (1, 32, 14),   # a 512^2 input
    (2, 64, 14),   # MedSAM: 25 windows, 4900 windowed rows for 4096 tokens
]
PADDED_GEOMETRIES = [geo for geo in GEOMETRIES if geo[1] % geo[2]]


def window_rows(batch, g, ws):
    nw = -(-g // ws)
    return batch * nw * nw * ws * ws


def window_index(batch, g, ws):
    """(idx, valid): for every row r of the window-partition order of `batch` g x g grids in ws x ws windows, idx[r] is the
    token-order row (b*g + y)*g + x it holds, or -1 where valid[r] is False (a padding row of a border window)."""
    nw = -(-g // ws)
    b, wy, wx, j, i = torch.meshgrid(torch.arange(batch), torch.arange(nw), torch.arange(nw), torch.arange(ws),
                                     torch.arange(ws), indexing="ij")
    y, x = wy * ws + j, wx * ws + i
    valid = ((y < g) & (x < g)).reshape(-1)
    idx = ((b * g + y) * g + x).reshape(-1)
    return torch.where(valid, idx, torch.full_like(idx, -1)), valid


def token_to_window(batch, g, ws):
    """inv[t]: the windowed row that holds token-order row t (every token sits in exactly one)."""
    idx, valid = window_index(batch, g, ws)
    inv = torch.full((batch * g * g,), -1, dtype=torch.int64)
    inv[idx[valid]] = torch.nonzero(valid).reshape(-1)
    assert int(inv.min()) >= 0
    return inv


# the byte offsets of an MX tensor's scales: restated once, in oracle/mx_designs.py
from oracle.mx_designs import mx_rows_pad, mx_scale_offsets  # noqa: E402,F401


def token_code_rows(tokens, D):
    """Designed LayerNorm input [tokens, D] (small integers, exact in bf16): row t = offset_t + s_k(t) * p_c, where the D
    columns form 16 groups k of D / 16, s_k(t) = +1 / -1 is bit k of t and p_c = +1, -1, +1, ... inside a group.  Every
    group sums to zero, so the row mean is offset_t exactly and LayerNorm (gamma 1, beta 0) gives s_k(t) p_c / sqrt(1 + eps):
    the signs of a normalised row spell its token number, whatever row of the output it was written to."""
    assert D % 32 == 0 and tokens <= 1 << 16
    w = D // 16
    t = torch.arange(tokens)
    bits = ((t[:, None] >> torch.arange(16)[None, :]) & 1) * 2 - 1          # [tokens, 16]
    p = 1 - 2 * (torch.arange(w) % 2)                                        # [w]
    off = (t % 7 - 3)[:, None, None]
    return (off + bits[:, :, None] * p[None, None, :]).reshape(tokens, D).float()


def decode_token_code(y, D):
    """Token numbers spelled by the signs of normalised token_code_rows rows y [rows, D] (any float dtype)."""
    w = D // 16
    first = y.reshape(y.shape[0], 16, w)[:, :, 0].double()                   # p_c = +1 there
    return ((first > 0).long() << torch.arange(16)[None, :]).sum(1)


def sparse_sign_weight(N, K, gen, nnz=16):
    """W [N, K] float: every row has at most nnz entries of +-1 at random columns, always including columns 0 and K - 1."""
    W = torch.zeros(N, K)
    cols = torch.randint(0, K, (N, nnz), generator=gen)
    cols[:, 0], cols[:, 1] = 0, K - 1
    sign = torch.randint(0, 2, (N, nnz), generator=gen).float() * 2 - 1
    W[torch.arange(N)[:, None], cols] = sign                                 # (a repeated column keeps one of its signs)
    assert int((W != 0).sum(1).max()) <= nnz and bool((W[:, 0] != 0).all()) and bool((W[:, -1] != 0).all())
    return W


def im2col3_ref(x_bits, batch, g):
    """3 x 3 / padding 1 im2col of NHWC int16 bit patterns [batch*g*g, C] -> [batch*g*g, 9*C], tap-major, through F.unfold:
    the patterns travel as float64 numbers (exact both ways) and the zero padding comes back as the pattern 0 = bf16 +0."""
    C = x_bits.shape[1]
    img = x_bits.reshape(batch, g, g, C).permute(0, 3, 1, 2).double()
    u = torch.nn.functional.unfold(img, kernel_size=3, padding=1)            # [batch, C*9, g*g], rows c*9 + ky*3 + kx
    u = u.reshape(batch, C, 9, g * g).permute(0, 3, 2, 1).reshape(batch * g * g, 9 * C)
    return u.to(torch.int16)
