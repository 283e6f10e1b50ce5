"""Single-operator entry points of libvdr.so (vdr_op_*), used by the per-kernel parity tests and
the kernel benchmark.  Every tensor must already live on the HIP device; nothing falls back."""
from __future__ import annotations

import torch

from . import _lib as L


def _s(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_dtype=torch.bfloat16, out=None):
    """`out`: write into this caller-owned tensor instead of a fresh one (x's shape, out_dtype, contiguous)."""
    lib = L.load()
    assert x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
    D = x.shape[-1]
    rows = x.numel() // D
    if out is None:
        y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    else:
        assert tuple(out.shape) == tuple(x.shape) and out.is_contiguous() and out.dtype == out_dtype and out.device == x.device
        y = out
    L.check(lib.vdr_op_layernorm(x.data_ptr(), 1 if x.dtype == torch.bfloat16 else 0, y.data_ptr(),
                                 1 if out_dtype == torch.bfloat16 else 0, gamma.data_ptr(), beta.data_ptr(), rows, D,
                                 float(eps), _s(x)))
    return y


def pack_linear_weight(W: torch.Tensor) -> torch.Tensor:
    """W [N, K] bf16 (PyTorch layout) -> the library's packed GEMM weight layout (what vdr_finalize builds for a
    model's weights): [N/2][K/32][2][32], returned as an [N, K]-shaped opaque tensor."""
    lib = L.load()
    assert W.is_cuda and W.dtype == torch.bfloat16 and W.is_contiguous() and W.dim() == 2
    Wp = torch.empty_like(W)
    L.check(lib.vdr_op_pack_linear_weight(W.data_ptr(), W.shape[0], W.shape[1], Wp.data_ptr(), _s(W)))
    return Wp


def linear(x, W, bias=None, resid=None, gamma=None, epilogue=L.EPI_BIAS, variant=0, out=None, packed=False):
    """x [M,K] bf16, W [N,K] bf16 (for EPI_SWIGLU W/bias must already be gate-pair packed: see pack_w12).
    packed=True: W is the result of pack_linear_weight (same values, whole-line operand loads)."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and x.is_contiguous() and W.is_contiguous()
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty((M, N // 2 if epilogue == L.EPI_SWIGLU else N), dtype=torch.bfloat16, device=x.device)
    fn = lib.vdr_op_linear_packed if packed else lib.vdr_op_linear
    L.check(fn(x.data_ptr(), W.data_ptr(), _p(bias), _p(resid), _p(gamma), out.data_ptr(), M, N, K, epilogue, variant, _s(x)))
    return out


def ln_fold_weights(W: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swiglu: bool = False):
    """The host fold of one linear behind a LayerNorm (vdr_ln_fold_weights): fp32 CPU W [N, K], b [N], gamma / beta [K]
    -> (Wf bf16 [N, K], colsum fp32 [N], tbias fp32 [N]), in gate-pair order when swiglu (W / b: mlp.w12 as PyTorch holds it)."""
    lib = L.load()
    W, b, gamma, beta = (t.detach().float().contiguous().cpu() for t in (W, b, gamma, beta))
    N, K = W.shape
    wf = torch.empty((N, K), dtype=torch.int16)
    cs = torch.empty(N, dtype=torch.float32)
    tb = torch.empty(N, dtype=torch.float32)
    L.check(lib.vdr_ln_fold_weights(W.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), N, K, int(swiglu),
                                    wf.data_ptr(), cs.data_ptr(), tb.data_ptr()))
    return wf.view(torch.bfloat16), cs, tb


def linear_ln_stats(x, W, bias, resid, part, variant, gamma=None, out=None, resid32=None, out32=None, stats=None,
                    counters=None, eps=1e-6):
    """The residual linear of the LayerNorm fold (vdr_op_linear_ln_stats): out = resid + gamma * (x W^T + bias) (fp32 stream:
    resid32 / out32), plus the (sum, sumsq) partials of out's bf16 rows in part [N/64, part_stride, 2]; with stats /
    counters also (mean, rstd) [M, 2] finalised by the GEMM's last workgroup per row block."""
    lib = L.load()
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    L.check(lib.vdr_op_linear_ln_stats(x.data_ptr(), W.data_ptr(), _p(bias), _p(resid), _p(gamma), out.data_ptr(),
                                       _p(resid32), _p(out32), M, N, K, variant, part.data_ptr(), part.shape[1],
                                       _p(stats), _p(counters), float(eps), _s(x)))
    return out


def ln_finalize(part: torch.Tensor, rows: int, eps: float, stats=None):
    """(sum, sumsq) partials [D/64, stride, 2] -> (mean, rstd) [rows, 2] (vdr_op_ln_finalize)"""
    lib = L.load()
    if stats is None:
        stats = torch.empty((rows, 2), dtype=torch.float32, device=part.device)
    L.check(lib.vdr_op_ln_finalize(part.data_ptr(), part.shape[1], rows, part.shape[0] * 64, float(eps), stats.data_ptr(),
                                   _s(part)))
    return stats


def linear_ln_fold(x, Wf, colsum, tbias, variant, epilogue=L.EPI_BIAS, stats=None, part=None, M=None, eps=1e-6, out=None):
    """The consumer of the LayerNorm fold (vdr_op_linear_ln_fold): epi(rstd (x Wf^T - mean colsum) + tbias) with (mean,
    rstd) from stats [>= M, 2] or finalised in the GEMM from part.  M defaults to x's rows; x (and stats) may hold more
    rows than M: they are readable padding (the 8-phase variant reads a ragged last tile whole)."""
    lib = L.load()
    rows, K = x.shape
    M = rows if M is None else M
    N = Wf.shape[0]
    if out is None:
        out = torch.empty((M, N // 2 if epilogue == L.EPI_SWIGLU else N), dtype=torch.bfloat16, device=x.device)
    x_rows = rows if stats is None else min(rows, stats.shape[0])
    L.check(lib.vdr_op_linear_ln_fold(x.data_ptr(), Wf.data_ptr(), colsum.data_ptr(), tbias.data_ptr(), _p(stats), _p(part),
                                      0 if part is None else part.shape[1], out.data_ptr(), M, N, K, x_rows, float(eps),
                                      epilogue, variant, _s(x)))
    return out


class MxTensor:
    """e4m3 payload [rows, K] (uint8) + e8m0 block scales in the device layout of csrc/mx.hip."""

    def __init__(self, q: torch.Tensor, scales: torch.Tensor):
        self.q, self.scales = q, scales

    @property
    def shape(self):
        return self.q.shape

    @staticmethod
    def empty(rows: int, K: int, device):
        lib = L.load()
        return MxTensor(torch.empty((rows, K), dtype=torch.uint8, device=device),
                        torch.zeros(int(lib.vdr_mx_scale_bytes(rows, K)), dtype=torch.uint8, device=device))

    def dequantize(self) -> torch.Tensor:
        lib = L.load()
        rows, K = self.q.shape
        y = torch.empty((rows, K), dtype=torch.float32, device=self.q.device)
        L.check(lib.vdr_op_mx_dequantize(self.q.data_ptr(), self.scales.data_ptr(), rows, K, y.data_ptr(), _s(self.q)))
        return y


def _mx_out(out, rows: int, K: int, device) -> MxTensor:
    if out is None:
        return MxTensor.empty(rows, K, device)
    assert tuple(out.q.shape) == (rows, K) and out.q.is_contiguous() and out.q.dtype == torch.uint8
    assert out.scales.numel() == int(L.load().vdr_mx_scale_bytes(rows, K)) and out.scales.is_contiguous()
    return out


def mx_quantize(x: torch.Tensor, out: MxTensor = None) -> MxTensor:
    """bf16 [rows, K] -> MX-fp8 (block 32 along K); `out`: write into this MxTensor (scale bytes of no valid row keep
    what they hold)."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[1] % 32 == 0
    rows, K = x.shape
    t = _mx_out(out, rows, K, x.device)
    L.check(lib.vdr_op_mx_quantize(x.data_ptr(), rows, K, t.q.data_ptr(), t.scales.data_ptr(), _s(x)))
    return t


def layernorm_mx(x: torch.Tensor, gamma, beta, eps: float, out: MxTensor = None) -> MxTensor:
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()
    rows, D = x.shape
    t = _mx_out(out, rows, D, x.device)
    L.check(lib.vdr_op_layernorm_mx(x.data_ptr(), gamma.float().contiguous().data_ptr(), beta.float().contiguous().data_ptr(),
                                    float(eps), rows, D, t.q.data_ptr(), t.scales.data_ptr(), _s(x)))
    return t


def linear_mx(x: MxTensor, W: MxTensor, bias=None, resid=None, gamma=None, epilogue=L.EPI_BIAS, variant=0, mx_out=False,
              out=None):
    """MX x [M,K] . MX W [N,K]^T on the block-scaled fp8 MFMA; returns bf16 [M,N] or (mx_out) an MxTensor.  `out`: the
    tensor (mx_out: MxTensor) to write into; it may be `resid` itself, as in the forward."""
    lib = L.load()
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K
    No = N // 2 if epilogue == L.EPI_SWIGLU else N
    if mx_out:
        out = _mx_out(out, M, No, x.q.device)
        yp, ysp = out.q.data_ptr(), out.scales.data_ptr()
    else:
        if out is None:
            out = torch.empty((M, No), dtype=torch.bfloat16, device=x.q.device)
        assert tuple(out.shape) == (M, No) and out.dtype == torch.bfloat16 and out.is_contiguous()
        yp, ysp = out.data_ptr(), None
    L.check(lib.vdr_op_linear_mx(x.q.data_ptr(), x.scales.data_ptr(), W.q.data_ptr(), W.scales.data_ptr(), _p(bias),
                                 _p(resid), _p(gamma), yp, ysp, M, N, K, epilogue, variant, _s(x.q)))
    return out


def pack_w12(w12: torch.Tensor, b12: torch.Tensor):
    """Interleave SwiGLU x1/x2 rows in blocks of 32 (the layout vdr_set_weight builds for mlp.w12)."""
    F2 = w12.shape[0]
    F = F2 // 2
    assert F % 32 == 0
    idx = torch.arange(F2)
    blk, t = idx // 64, idx % 64
    src = torch.where(t < 32, blk * 32 + t, F + blk * 32 + (t - 32))
    return w12[src].contiguous(), b12[src].contiguous()


def attention(qkv: torch.Tensor, batch: int, seq: int, heads: int, variant=0, head_dim=64, lengths=None, len_add=0):
    """softmax(q k^T / sqrt(head_dim)) v per (batch entry, head) over a packed [batch*seq, 3*heads*head_dim] bf16
    activation (columns [q | k | v], each [heads, head_dim]); head_dim in {32, 64, 96, 128}.
    lengths (int [batch]): entry b attends over its first min(seq, lengths[b] + len_add) rows only; the output rows
    past that length are undefined."""
    lib = L.load()
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    assert qkv.shape == (batch * seq, 3 * heads * head_dim)
    out = torch.empty((batch * seq, heads * head_dim), dtype=torch.bfloat16, device=qkv.device)
    if lengths is not None:
        lens = torch.as_tensor(lengths, dtype=torch.int32)
        if lens.shape != (batch,) or int(lens.min()) + len_add < 1:
            raise ValueError("lengths must be [batch] with lengths[b] + len_add >= 1")
        lens = lens.to(qkv.device).contiguous()
        L.check(lib.vdr_op_attention_varlen(qkv.data_ptr(), out.data_ptr(), batch, seq, heads, head_dim, lens.data_ptr(),
                                            len_add, variant, _s(qkv)))
    elif head_dim == 64:
        L.check(lib.vdr_op_attention(qkv.data_ptr(), out.data_ptr(), batch, seq, heads, variant, _s(qkv)))
    else:
        L.check(lib.vdr_op_attention_hd(qkv.data_ptr(), out.data_ptr(), batch, seq, heads, head_dim, variant, _s(qkv)))
    return out


def attention_pool(q: torch.Tensor, kv: torch.Tensor, batch: int, n: int, heads: int, head_dim: int = 64) -> torch.Tensor:
    """One-query attention pooling (vdr_op_attention_pool; SigLIP's pooling head): q fp32 [heads * head_dim], the
    projected probe shared by the batch; kv bf16 [batch * n, >= 2 * heads * head_dim], columns [k | v], rows may be
    strided (a column slice of a wider matrix).  Returns bf16 [batch, heads * head_dim]:
    out[b, h] = softmax_j(q_h . k[b, j, h] / sqrt(head_dim)) v[b, j, h].  head_dim in {32, 64, 96, 128}, n >= 1."""
    lib = L.load()
    D = heads * head_dim
    assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.numel() == D
    assert kv.is_cuda and kv.dtype == torch.bfloat16 and kv.dim() == 2 and kv.stride(1) == 1
    assert kv.shape[0] == batch * n and kv.shape[1] >= 2 * D
    out = torch.empty((batch, D), dtype=torch.bfloat16, device=kv.device)
    L.check(lib.vdr_op_attention_pool(q.data_ptr(), kv.data_ptr(), kv.stride(0), out.data_ptr(), batch, n, heads, head_dim, _s(kv)))
    return out


def attention_probs(qkv: torch.Tensor, batch: int, seq: int, heads: int, head_dim=64, q_rows=None, head_mean=False,
                    out_dtype=torch.float32):
    """The attention map of the same packed qkv: softmax(q k^T / sqrt(head_dim)) of the first q_rows query rows (None:
    all seq) of every (batch entry, head), normalised.  Returns [batch, heads, q_rows, seq], or [batch, q_rows, seq] with
    head_mean (the mean over the heads); float32 or bfloat16."""
    lib = L.load()
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    assert qkv.shape == (batch * seq, 3 * heads * head_dim)
    q_rows = seq if q_rows is None else int(q_rows)
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    shape = (batch, q_rows, seq) if head_mean else (batch, heads, q_rows, seq)
    out = torch.empty(shape, dtype=out_dtype, device=qkv.device)
    L.check(lib.vdr_op_attention_probs(qkv.data_ptr(), out.data_ptr(), batch, seq, heads, head_dim, q_rows, int(bool(head_mean)),
                                       L.VDR_BF16 if out_dtype == torch.bfloat16 else L.VDR_F32, _s(qkv)))
    return out


def _rows2d(t, name, cols=None):
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)):
        raise TypeError(f"{name} must be a 2-D bfloat16 tensor on the HIP device with contiguous columns")
    if cols is not None and t.shape[1] != cols:
        raise ValueError(f"{name} has {t.shape[1]} columns, expected {cols}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def cross_attention(q, k, v, problems: int, tq: int, tk: int, heads: int, head_dim: int, q_add=None, k_add=None, out=None):
    """softmax(Q K^T / sqrt(head_dim)) v per (problem, head) with a handful of rows on one side (vdr_op_cross_attention): q
    [problems*tq, heads*head_dim], k and v [problems*tk, heads*head_dim] bf16, each contiguous or a column slice of a wider
    buffer (read in place); q_add [tq, heads*head_dim] / k_add [tk, heads*head_dim] fp32 tables added to every problem's q / k
    rows in fp32.  head_dim 16 or 32; tq <= 16 or tk <= 16.  Returns bf16 [problems*tq, heads*head_dim]."""
    lib = L.load()
    HD = heads * head_dim
    ldq, ldk, ldv = _rows2d(q, "q", HD), _rows2d(k, "k", HD), _rows2d(v, "v", HD)
    if q.shape[0] != problems * tq or k.shape[0] != problems * tk or v.shape[0] != problems * tk:
        raise ValueError("cross_attention: q must hold problems * tq rows, k and v problems * tk")
    for t, rows, name in ((q_add, tq, "q_add"), (k_add, tk, "k_add")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, HD)):
            raise ValueError(f"cross_attention: {name} must be a contiguous float32 [{rows}, {HD}] tensor on the device")
    if out is None:
        out = torch.empty((problems * tq, HD), dtype=torch.bfloat16, device=q.device)
    ldo = _rows2d(out, "out", HD)
    L.check(lib.vdr_op_cross_attention(q.data_ptr(), ldq, _p(q_add), k.data_ptr(), ldk, _p(k_add), v.data_ptr(), ldv,
                                       out.data_ptr(), ldo, problems, tq, tk, heads, head_dim, _s(q)))
    return out


def token_linear(x, W, bias=None, x_add=None, resid=None, relu=False, out=None, out_dtype=torch.bfloat16):
    """The token-side linear of the mask decoder (vdr_op_token_linear): x [M, K] bf16 (rows may be strided), W [N, K] or
    [groups, N, K] bf16 (row r uses group r % groups), bias fp32 [N] / [groups, N]; x_add: bf16(x + x_add) is the input;
    resid bf16 [M, N] is added after the ReLU.  One fp32 fma chain over k.  Returns [M, N] bf16 or fp32 (or writes `out`,
    which may be a column slice)."""
    lib = L.load()
    ldx = _rows2d(x, "x")
    M, K = x.shape
    if not (W.is_cuda and W.dtype == torch.bfloat16 and W.is_contiguous() and W.dim() in (2, 3) and W.shape[-1] == K):
        raise ValueError("token_linear: W must be a contiguous bfloat16 [N, K] or [groups, N, K] tensor")
    groups = W.shape[0] if W.dim() == 3 else 1
    N = W.shape[-2]
    if bias is not None and not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == groups * N):
        raise ValueError("token_linear: bias must be contiguous float32 [groups, N]")
    ldxa = _rows2d(x_add, "x_add", K) if x_add is not None else 0
    ldr = _rows2d(resid, "resid", N) if resid is not None else 0
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    if not (out.dim() == 2 and tuple(out.shape) == (M, N) and out.dtype in (torch.float32, torch.bfloat16) and (N == 1 or out.stride(1) == 1)):
        raise ValueError("token_linear: out must be [M, N] float32 or bfloat16 with contiguous columns")
    ldy = out.stride(0) if M > 1 else max(N, out.stride(0))
    L.check(lib.vdr_op_token_linear(x.data_ptr(), ldx, _p(x_add), ldxa, W.data_ptr(), _p(bias), _p(resid), ldr, out.data_ptr(),
                                    L.VDR_BF16 if out.dtype == torch.bfloat16 else L.VDR_F32, ldy, M, N, K, groups, int(bool(relu)),
                                    _s(x)))
    return out


def mask_upscale(x, W, bias, hyper, problems: int, g: int, gelu_in: bool = True, out=None):
    """The fused tail of the mask decoder (vdr_op_mask_upscale): x [problems*g*g*4, 64] bf16 LayerNorm2d rows, W [128, 64] bf16
    (row (dy*2+dx)*32 + c), bias fp32 [32], hyper fp32 [problems, 4, 32] -> low-resolution logits fp32 [problems, 4, 4g, 4g]."""
    lib = L.load()
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and tuple(x.shape) == (problems * g * g * 4, 64)):
        raise ValueError("mask_upscale: x must be a contiguous bfloat16 [problems*g*g*4, 64] tensor on the device")
    if not (W.dtype == torch.bfloat16 and W.is_contiguous() and tuple(W.shape) == (128, 64)):
        raise ValueError("mask_upscale: W must be contiguous bfloat16 [128, 64]")
    if not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == 32):
        raise ValueError("mask_upscale: bias must be float32 [32]")
    if not (hyper.dtype == torch.float32 and hyper.is_contiguous() and tuple(hyper.shape) == (problems, 4, 32)):
        raise ValueError("mask_upscale: hyper must be contiguous float32 [problems, 4, 32]")
    if out is None:
        out = torch.empty((problems, 4, 4 * g, 4 * g), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_mask_upscale(x.data_ptr(), W.data_ptr(), bias.data_ptr(), hyper.data_ptr(), out.data_ptr(), problems, g,
                                    int(bool(gelu_in)), _s(x)))
    return out


def mask_embed(emb, mask, weights, problems_per_image: int = 1, eps: float = 1e-6, out=None):
    """The fused keys of a decode with a mask prompt (vdr_op_mask_embed): emb fp32 [B, 256, g, g] (a channel-first view of a
    [B, g, g, 256] tensor is read in place), mask fp32 [B * problems_per_image, 4g, 4g], or [B, 4g, 4g] shared by the image's
    problems; weights fp32 [4684], mask_downscaling's ten tensors back to back (0.weight, 0.bias, 1.weight, 1.bias, 3.weight,
    3.bias, 4.weight, 4.bias, 6.weight, 6.bias) -> keys bf16 [B * problems_per_image * g * g, 256] = bf16(emb + dense)."""
    lib = L.load()
    if not (emb.is_cuda and emb.dtype == torch.float32 and emb.dim() == 4 and emb.shape[1] == 256 and emb.shape[2] == emb.shape[3]):
        raise ValueError("mask_embed: emb must be a float32 [B, 256, g, g] tensor on the device")
    B, g, nb = int(emb.shape[0]), int(emb.shape[2]), int(problems_per_image)
    if emb.permute(0, 2, 3, 1).is_contiguous():
        channels_last = 1
    else:
        emb, channels_last = emb.contiguous(), 0
    P = B * nb
    if not (mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous() and mask.dim() == 3 and tuple(mask.shape[1:]) == (4 * g, 4 * g)
            and mask.shape[0] in (P, B)):
        raise ValueError(f"mask_embed: mask must be a contiguous float32 [{P} or {B}, {4 * g}, {4 * g}] tensor on the device")
    per_image = int(mask.shape[0] != P)
    if not (weights.is_cuda and weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() == L.MASK_EMBED_WEIGHTS):
        raise ValueError(f"mask_embed: weights must be a contiguous float32 tensor of {L.MASK_EMBED_WEIGHTS} values on the device")
    if out is None:
        out = torch.empty((P * g * g, 256), dtype=torch.bfloat16, device=emb.device)
    if not (out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == P * g * g * 256):
        raise ValueError("mask_embed: out must be a contiguous bfloat16 [P * g * g, 256] tensor")
    L.check(lib.vdr_op_mask_embed(emb.data_ptr(), channels_last, mask.data_ptr(), per_image, weights.data_ptr(), out.data_ptr(), P, nb, g,
                                  float(eps), _s(emb)))
    return out


def mask_box(logits, prev, img: int, margin: float = 0.0, threshold: float = 0.0):
    """The box of each logit map (vdr_op_mask_box): logits fp32 [P, H, W] -- contiguous planes, the planes themselves may be
    strided, as token 0 of a [P, 4, H, W] tensor -- and prev fp32 [P, 4] -> (boxes fp32 [P, 4] (x0, y0, x1, y1) in pixels of the
    img x img input, grown by `margin` and clamped to [0, img]; area int32 [P]).  An empty mask returns prev's box and area 0."""
    lib = L.load()
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3):
        raise ValueError("mask_box: logits must be a float32 [P, H, W] tensor on the device")
    P, H, W = (int(v) for v in logits.shape)
    if not ((W == 1 or logits.stride(2) == 1) and (H == 1 or logits.stride(1) == W)):
        logits = logits.contiguous()
    stride = logits.stride(0) if P > 1 else H * W
    if stride < H * W:
        logits, stride = logits.contiguous(), H * W
    if not (prev.is_cuda and prev.dtype == torch.float32 and prev.is_contiguous() and tuple(prev.shape) == (P, 4)):
        raise ValueError(f"mask_box: prev must be a contiguous float32 [{P}, 4] tensor on the device")
    boxes = torch.empty((P, 4), dtype=torch.float32, device=logits.device)
    area = torch.empty((P,), dtype=torch.int32, device=logits.device)
    L.check(lib.vdr_op_mask_box(logits.data_ptr(), stride, prev.data_ptr(), boxes.data_ptr(), area.data_ptr(), P, H, W, int(img), float(margin),
                                float(threshold), _s(logits)))
    return boxes, area


MASK_STATS_MAX_SIDE, MASK_STATS_MAX_OUT, NMS_MAX_BOXES = 256, 4096, 4096  # VDR_MASK_STATS_MAX_SIDE, .._MAX_OUT, VDR_NMS_MAX_BOXES (include/vdr.h)


class PlaneOperand:
    """Planes of fp32 logits as vdr_op_mask_stats reads them (the operand builder of mask_stats): the tensor kept alive and
    (planes, planes_per_group, plane_stride, group_stride, H, W).  [P, H, W] or [G, M, H, W] on the device; a plane must be
    contiguous, the planes and groups may be strided (one token, or tokens 1 .. 3, of a [P, 4, H, W] tensor are read in place);
    anything else is copied once."""

    def __init__(self, x, op: str, name: str = "logits"):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() not in (3, 4):
            raise ValueError(f"{op}: {name} must be a float32 [P, H, W] or [G, M, H, W] tensor")
        if not x.is_cuda:
            raise ValueError(f"{op}: {name} must live on the HIP device")
        self.lead = tuple(int(v) for v in x.shape[:-2])  # the leading shape of every result: (P,) or (G, M)
        if x.dim() == 3:
            x = x.unsqueeze(1)
        G, M, H, W = (int(v) for v in x.shape)
        if min(G, M) < 1 or not (1 <= H <= MASK_STATS_MAX_SIDE and 1 <= W <= MASK_STATS_MAX_SIDE):
            raise ValueError(f"{op}: {name} needs at least one plane of 1 .. {MASK_STATS_MAX_SIDE} rows and columns, got {tuple(x.shape)}")
        if G * M > 65535:
            raise ValueError(f"{op}: at most 65535 planes a call, got {G * M}")
        ps, gs = (x.stride(1) if M > 1 else H * W), (x.stride(0) if G > 1 else M * H * W)
        ok = (W == 1 or x.stride(3) == 1) and (H == 1 or x.stride(2) == W) and ps >= H * W and gs >= (M - 1) * ps + H * W
        if not ok:
            x = x.contiguous()
            ps, gs = H * W, M * H * W
        self.x, self.planes, self.group, self.plane_stride, self.group_stride, self.H, self.W = x, G * M, M, ps, gs, H, W


def _workspace(workspace, need: int, device):
    """the caller's workspace, or a fresh one of the library's byte count (the C entry point checks a given one's size)"""
    return torch.empty((need,), dtype=torch.uint8, device=device) if workspace is None else workspace


def _result(op: str, name: str, t, shape, dtype, device):
    """the caller's tensor to write `name` into, checked, or a fresh one"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (isinstance(t, torch.Tensor) and t.device == device and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{op}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the operand's device")
    return t


def check_out_size(op: str, size) -> "tuple[int, int]":
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{op}: size must be (height, width), got {size!r}") from None
    if not (1 <= oh <= MASK_STATS_MAX_OUT and 1 <= ow <= MASK_STATS_MAX_OUT):
        raise ValueError(f"{op}: size must be 1 .. {MASK_STATS_MAX_OUT} in both directions, got {size!r}")
    return oh, ow


def mask_stats(logits, size, threshold: float = 0.0, offset: float = 1.0, workspace=None):
    """The statistics of candidate masks at image resolution (vdr_op_mask_stats): logits fp32 [P, H, W] or [G, M, H, W] on the
    device (PlaneOperand: strided planes are read in place) -> (counts int32 [.., 3], box int32 [.., 4]) of the bilinear
    (align_corners=False) up-sampling to size = (oh, ow), which is never written: the pixel counts above threshold + offset,
    threshold and threshold - offset, and (min x, min y, max x, max y) of the pixels above threshold (0, 0, 0, 0 for none).
    Bit for bit vdr.amg.mask_stats_torch.  workspace: a uint8 device tensor of at least vdr_mask_stats_workspace_bytes."""
    o = PlaneOperand(logits, "mask_stats")
    oh, ow = check_out_size("mask_stats", size)
    if not float(offset) >= 0.0:
        raise ValueError(f"mask_stats: offset must be >= 0, got {offset!r}")
    lib = L.load()
    dev = o.x.device
    workspace = _workspace(workspace, lib.vdr_mask_stats_workspace_bytes(o.planes, o.H, o.W, oh, ow), dev)
    counts = torch.empty((*o.lead, 3), dtype=torch.int32, device=dev)
    box = torch.empty((*o.lead, 4), dtype=torch.int32, device=dev)
    L.check(lib.vdr_op_mask_stats(o.x.data_ptr(), o.plane_stride, o.group, o.group_stride, o.planes, o.H, o.W, oh, ow, float(threshold),
                                  float(offset), workspace.data_ptr(), workspace.numel(), counts.data_ptr(), box.data_ptr(), _s(o.x)))
    return counts, box


def nms(boxes, scores, iou_threshold: float, workspace=None):
    """Greedy box non-maximum suppression (vdr_op_nms; torchvision's definition, bit for bit vdr.amg.nms_torch): boxes [N, 4]
    (x0, y0, x1, y1) and scores [N] on the device, N in 1 .. 4096 -> (kept int32 [N]: the kept box indices best first, then -1;
    count int32 [1]), both on the device: nothing here synchronises.  Boxes are visited in the order of a stable descending
    sort of the scores (equal scores: the lower index first); a box goes when an earlier kept box has IoU > iou_threshold."""
    if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda and boxes.dim() == 2 and boxes.shape[1] == 4 and 1 <= boxes.shape[0] <= NMS_MAX_BOXES):
        raise ValueError(f"nms: boxes must be an [N, 4] tensor on the device, N in 1 .. {NMS_MAX_BOXES}")
    N = int(boxes.shape[0])
    if not (isinstance(scores, torch.Tensor) and scores.device == boxes.device and tuple(scores.shape) == (N,)):
        raise ValueError(f"nms: scores must be [{N}] on the boxes' device")
    if float(iou_threshold) != float(iou_threshold):
        raise ValueError("nms: iou_threshold must be a number")
    lib = L.load()
    dev = boxes.device
    bx = boxes.to(torch.float32).contiguous()
    order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32)
    workspace = _workspace(workspace, lib.vdr_nms_workspace_bytes(N), dev)
    keep = torch.empty((N,), dtype=torch.uint8, device=dev)
    kept = torch.empty((N,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    L.check(lib.vdr_op_nms(bx.data_ptr(), order.data_ptr(), N, float(iou_threshold), workspace.data_ptr(), workspace.numel(), keep.data_ptr(),
                           kept.data_ptr(), count.data_ptr(), _s(bx)))
    return kept, count


def mask_binarize(logits, size, threshold: float = 0.0, out=None):
    """Candidate masks at image resolution (vdr_op_mask_binarize): logits fp32 [P, H, W] or [G, M, H, W] on the device
    (PlaneOperand: strided planes are read in place) -> uint8 [.., oh, ow], 1 where the bilinear (align_corners=False)
    up-sampling to size = (oh, ow) is > threshold.  The arithmetic is mask_stats': the set pixels are the ones it counts and
    boxes; bit for bit vdr.amg.upsample_torch(logits, size) > threshold."""
    o = PlaneOperand(logits, "mask_binarize")
    oh, ow = check_out_size("mask_binarize", size)
    if float(threshold) != float(threshold):
        raise ValueError("mask_binarize: threshold must be a number")
    lib = L.load()
    dev = o.x.device
    out = _result("mask_binarize", "out", out, (*o.lead, oh, ow), torch.uint8, dev)
    workspace = _workspace(None, lib.vdr_mask_binarize_workspace_bytes(o.planes, o.H, o.W, oh, ow), dev)
    L.check(lib.vdr_op_mask_binarize(o.x.data_ptr(), o.plane_stride, o.group, o.group_stride, o.planes, o.H, o.W, oh, ow, float(threshold),
                                     workspace.data_ptr(), workspace.numel(), out.data_ptr(), _s(o.x)))
    return out


def _mask_planes(mask, op: str):
    from . import components as cc
    m, single = cc.as_planes(mask, op)
    if not m.is_cuda:
        raise ValueError(f"{op}: mask must live on the HIP device")
    return m, single


def connected_components(mask, connectivity: int = 8, value: int = 1, workspace=None):
    """Connected components of mask planes (vdr_op_connected_components): mask bool or uint8 [P, H, W] or [H, W] on the device
    (nonzero = set), connectivity 4 or 8, value 1 (components of the set pixels) or 0 (of the clear pixels) -> (root int32
    like mask: the lowest pixel index y * W + x of each pixel's component, -1 where not selected; area int32 like mask: the
    component's pixel count at its root, 0 elsewhere; count int32 [P]).  Bit for bit vdr.components.label_torch; nothing here
    synchronises."""
    from . import components as cc
    m, single = _mask_planes(mask, "connected_components")
    cc.check_connectivity("connected_components", connectivity)
    if isinstance(value, bool) or value not in (0, 1):
        raise ValueError(f"connected_components: value must be 0 or 1, got {value!r}")
    lib = L.load()
    P, H, W = (int(v) for v in m.shape)
    workspace = _workspace(workspace, lib.vdr_connected_components_workspace_bytes(P, H, W), m.device)
    root = torch.empty((P, H, W), dtype=torch.int32, device=m.device)
    area = torch.empty((P, H, W), dtype=torch.int32, device=m.device)
    count = torch.empty((P,), dtype=torch.int32, device=m.device)
    L.check(lib.vdr_op_connected_components(m.data_ptr(), P, H, W, int(connectivity), int(value), workspace.data_ptr(), workspace.numel(),
                                            root.data_ptr(), area.data_ptr(), count.data_ptr(), _s(m)))
    return (root[0], area[0], count) if single else (root, area, count)


def mask_clean(mask, min_area: int = 0, holes: bool = False, islands: bool = False, largest: bool = False, connectivity: int = 8, workspace=None,
               out=None, changed=None, stats=None):
    """Small-region removal / keep-largest on mask planes (vdr_op_mask_clean): mask bool or uint8 [P, H, W] or [H, W] on the
    device -> (out uint8 like mask, 0 / 1; changed int32 [P]: bit 0 the hole step changed the plane, bit 1 the island / largest
    step; stats int32 [P, 5]: area and inclusive box x0, y0, x1, y1 of out, zeros for an empty plane).  holes: components of
    the clear pixels below min_area become set; then islands: components of the set pixels below min_area are cleared (the
    largest stays if all are below); or largest: only the largest component stays (ties: the lowest root).  Bit for bit
    vdr.components.clean_torch; nothing here synchronises.  out / changed / stats: contiguous device tensors of those shapes and
    types to write into (a slice of a larger result, say) instead of fresh ones; out may not share memory with mask."""
    from . import components as cc
    m, single = _mask_planes(mask, "mask_clean")
    min_area, mode, connectivity = cc.check_clean("mask_clean", min_area, holes, islands, largest, connectivity)
    lib = L.load()
    P, H, W = (int(v) for v in m.shape)
    workspace = _workspace(workspace, lib.vdr_mask_clean_workspace_bytes(P, H, W), m.device)
    out = _result("mask_clean", "out", out, (P, H, W), torch.uint8, m.device)
    changed = _result("mask_clean", "changed", changed, (P,), torch.int32, m.device)
    stats = _result("mask_clean", "stats", stats, (P, 5), torch.int32, m.device)
    L.check(lib.vdr_op_mask_clean(m.data_ptr(), P, H, W, min_area, connectivity, mode, workspace.data_ptr(), workspace.numel(), out.data_ptr(),
                                  changed.data_ptr(), stats.data_ptr(), _s(m)))
    return (out[0] if single else out), changed, stats


def distance_transform(mask, value: int = 1, outside: bool = False, return_nearest: bool = False, return_peak: bool = False, threshold=None,
                       workspace=None, return_d2: bool = True):
    """Exact Euclidean distance transform of mask planes (vdr_op_distance_transform): mask bool or uint8 [P, H, W] or [H, W] on
    the device (nonzero = set), value 1 (the set pixels are measured) or 0 (the clear ones) -> d2 int32 like mask: the squared
    distance to the nearest pixel that is not selected, 0 where not selected, 2^31 - 1 where there is none; outside=True counts
    everything beyond the plane as not selected.  return_nearest adds nearest int32 like mask (the lowest index y * W + x of a
    nearest non-selected pixel, -1 where there is none; not with outside), return_peak adds peak int32 [P, 2] (the largest d2
    and the lowest index that attains it, (0, -1) for a plane with nothing selected); with either the result is a tuple in
    that order.  threshold = r2 (an integer >= 0): the first result is the uint8 plane d2 <= r2 INSTEAD of d2, and the int32
    plane is never written.  return_d2=False leaves the first result out altogether (no plane of the mask's size is allocated
    or written; not together with threshold, and something else must be asked for): vdr.morphology.inner_point asks for the
    peak alone.  Bit for bit vdr.morphology.edt_torch; nothing here synchronises.  Every refusal of an argument comes before
    the device is asked for."""
    from . import components as cc
    from . import morphology as mo
    cc.as_planes(mask, "distance_transform")
    value, outside, r2 = mo.check_edt("distance_transform", value, outside, return_nearest, threshold)
    if not return_d2 and (r2 is not None or not (return_nearest or return_peak)):
        raise ValueError("distance_transform: return_d2=False goes with return_nearest or return_peak and without threshold")
    m, single = _mask_planes(mask, "distance_transform")
    lib = L.load()
    P, H, W = (int(v) for v in m.shape)
    workspace = _workspace(workspace, lib.vdr_distance_transform_workspace_bytes(P, H, W), m.device)
    first = torch.empty((P, H, W), dtype=torch.int32 if r2 is None else torch.uint8, device=m.device) if return_d2 else None
    nearest = torch.empty((P, H, W), dtype=torch.int32, device=m.device) if return_nearest else None
    peak = torch.empty((P, 2), dtype=torch.int32, device=m.device) if return_peak else None
    L.check(lib.vdr_op_distance_transform(m.data_ptr(), P, H, W, value, outside, 0 if r2 is None else r2, workspace.data_ptr(), workspace.numel(),
                                          _p(first) if r2 is None else None, _p(nearest), _p(peak),
                                          _p(first) if r2 is not None else None, _s(m)))
    out = [first[0] if single else first] if return_d2 else []
    if return_nearest:
        out.append(nearest[0] if single else nearest)
    if return_peak:
        out.append(peak)
    return out[0] if len(out) == 1 else tuple(out)


def distance_transform_3d(vol, spacing=(1, 1, 1), value: int = 1, outside=False, return_peak: bool = False, threshold=None, return_d2: bool = True,
                          workspace=None):
    """Exact 3-D Euclidean distance transform of mask volumes under integer voxel spacing (vdr_op_distance_transform_3d): vol bool
    or uint8 [Z, H, W] or [P, Z, H, W] on the device (nonzero = set), spacing three integers (qz, qy, qx) in 1 .. 65535
    (vdr.morphology.quantize_spacing makes them from millimetres), value 1 (the set voxels are measured) or 0 (the clear ones) ->
    d2 int64 like vol: min (qz dz)^2 + (qy dy)^2 + (qx dx)^2 over the voxels that are not selected, 0 where not selected, 2^63 - 1
    where there is none.  outside: False, True or three bools (z, y, x) -- on a set axis everything beyond the volume's two faces
    counts as not selected.  return_peak adds peak int64 [P, 2] (the largest d2 and the lowest voxel index (z H + y) W + x that
    attains it, (0, -1) for a volume with nothing selected).  threshold = r2 (an integer >= 0): the first result is the uint8
    volume d2 <= r2 INSTEAD of d2; no int64 volume is written, and asked for alone it lets the searches end after O(r) steps.
    return_d2=False leaves the first result out (with return_peak, without threshold).  Bit for bit
    vdr.morphology.edt3d_torch and rint(scipy.ndimage.distance_transform_edt(selected, sampling=spacing) ^ 2); nothing here
    synchronises.  Every refusal of an argument comes before the device is asked for."""
    from . import components as cc
    from . import morphology as mo
    v, single = cc.as_volumes(vol, "distance_transform_3d")
    q, value, bits, r2 = mo.check_edt3("distance_transform_3d", spacing, value, outside, threshold, v.shape[1:])
    if not return_d2 and (r2 is not None or not return_peak):
        raise ValueError("distance_transform_3d: return_d2=False goes with return_peak and without threshold")
    P, Z, H, W = (int(n) for n in v.shape)
    if not v.is_cuda:
        raise ValueError("distance_transform_3d: mask must live on the HIP device")
    lib = L.load()
    workspace = _workspace(workspace, lib.vdr_distance_transform_3d_workspace_bytes(P, Z, H, W), v.device)
    first = torch.empty((P, Z, H, W), dtype=torch.int64 if r2 is None else torch.uint8, device=v.device) if return_d2 else None
    peak = torch.empty((P, 2), dtype=torch.int64, device=v.device) if return_peak else None
    L.check(lib.vdr_op_distance_transform_3d(v.data_ptr(), P, Z, H, W, q[0], q[1], q[2], value, bits, 0 if r2 is None else r2, workspace.data_ptr(),
                                             workspace.numel(), _p(first) if r2 is None else None, _p(peak),
                                             _p(first) if r2 is not None else None, _s(v)))
    out = [first[0] if single else first] if return_d2 else []
    if return_peak:
        out.append(peak)
    return out[0] if len(out) == 1 else tuple(out)


def log_bin(x: torch.Tensor, gh: int, gw: int, hierarchy: int = 2, out_dtype=torch.float32, out=None) -> torch.Tensor:
    """Log-binning of a dense descriptor map (vdr_op_log_bin): x [B, gh*gw, C] bf16 or fp32 -- contiguous, or a view whose
    last dimension is contiguous, such as the key columns and patch rows buf[:, P:, C:2*C] of a [B, P + n, 3C] qkv
    activation, read in place -- -> [B, gh*gw, (1 + 8*hierarchy)*C]: per patch its own descriptor, its 8 neighbours, and
    for k = 1 .. hierarchy-1 the 8 neighbours at 3^k spacing of the 3^k x 3^k window means (edges clamped, windows cut to
    the grid).  fp32 sums, one IEEE division, one rounding to out_dtype; level-0 bins are copies."""
    lib = L.load()
    if not (x.is_cuda and x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16)):
        raise TypeError("log_bin: x must be a [B, gh*gw, C] float32 or bfloat16 tensor on the HIP device")
    B, n, Cc = x.shape
    if n != int(gh) * int(gw):
        raise ValueError(f"log_bin: x has {n} rows, the grid {gh} x {gw}")
    if Cc > 1 and x.stride(2) != 1:
        raise ValueError("log_bin: the channels of x must be contiguous")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    h = int(hierarchy)
    if not 1 <= h <= 3:
        raise ValueError(f"log_bin: hierarchy must be 1, 2 or 3, got {hierarchy}")
    ld = x.stride(1) if n > 1 else Cc
    image_stride = x.stride(0) if B > 1 else n * ld
    bins = 1 + 8 * h
    shape = (B, n, bins * Cc)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    elif out.dtype not in (torch.float32, torch.bfloat16) or out.device != x.device or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"log_bin: out must be a contiguous float32 or bfloat16 tensor of shape {shape} on {x.device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}")
    work = torch.empty((max(h - 1, 0) * B * n * Cc,), dtype=torch.float32, device=x.device) if h > 1 else None
    L.check(lib.vdr_op_log_bin(x.data_ptr(), L.VDR_BF16 if x.dtype == torch.bfloat16 else L.VDR_F32, ld, image_stride, B, int(gh),
                               int(gw), Cc, h, _p(work), out.data_ptr(), L.VDR_BF16 if out.dtype == torch.bfloat16 else L.VDR_F32,
                               _s(x)))
    return out


class DescOperand:
    """A descriptor map as the descriptor ops read it (the host side of check_desc_operand, csrc/vdr_api.hip): the tensor kept
    alive, its dtype code, its strides in elements and its shape (problems, imgs, t, d); R = imgs * t rows per problem.  Built
    by desc_operand; k-means builds it once per fit."""

    def __init__(self, x, ld, image_stride, problem_stride, problems, imgs, t, d):
        self.x, self.dtype = x, (L.VDR_BF16 if x.dtype == torch.bfloat16 else L.VDR_F32)
        self.ld, self.image_stride, self.problem_stride = ld, image_stride, problem_stride
        self.problems, self.imgs, self.t, self.d = problems, imgs, t, d
        self.R = imgs * t

    @property
    def stride(self):
        """of a [P, t, d] operand: the stride of its one level above the rows, images (joint) or problems"""
        return self.image_stride if self.imgs > 1 else self.problem_stride

    def work(self, k: int) -> torch.Tensor:
        """the scratch of the two k-means ops for k centroids"""
        n = L.load().vdr_kmeans_work_bytes(self.problems, self.imgs, self.t, self.d, int(k))
        return torch.empty((n,), dtype=torch.uint8, device=self.x.device)


def desc_operand(x, op: str, name: str = "x", joint: bool = False, keep_fp32: bool = False, max_d=None, four_d: bool = False,
                 refuse_strided_channels: bool = False) -> DescOperand:
    """The host-side refusals of a descriptor operand and its description for the library, for every descriptor op.  x
    [P, t, d] bf16 / fp32 on the device: one problem per image, or the P * t rows of all images as one problem with joint=True.
    It is read where it lies when its channels are contiguous and its rows, images and problems 16-byte aligned (a column
    slice of a wider buffer, rows behind a prefix, a stride of 0 from expand()), and copied once otherwise.  d must be a
    multiple of 32.  What the families differ in:
      keep_fp32                fp32 stays fp32 (PCA, the Gram side); otherwise it is rounded once to bf16
      max_d                    the widest d taken (PCA: 2048)
      four_d                   [problems, imgs, t, d] is taken as it says, and a DescOperand is passed through (k-means, Mahalanobis)
      refuse_strided_channels  channels that are not contiguous are a ValueError, not a copy (nn_cosine, affinity_bits)"""
    if four_d and isinstance(x, DescOperand):
        return x
    if not isinstance(x, torch.Tensor) or x.dim() not in ((3, 4) if four_d else (3,)) or x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{op}: {name} must be a [P, t, d] {'or [problems, imgs, t, d] ' if four_d else ''}float32 or bfloat16 tensor")
    if not x.is_cuda:
        raise TypeError(f"{op}: {name} must live on the HIP device")
    if x.dim() == 3:
        x = x.unsqueeze(0) if joint else x.unsqueeze(1)
    elif joint:
        raise ValueError(f"{op}: joint=True goes with a [P, t, d] operand")
    problems, imgs, t, d = x.shape
    if min(problems, imgs, t, d) <= 0:
        raise ValueError(f"{op}: empty operand")
    if d % 32 or (max_d and d > max_d):
        raise ValueError(f"{op}: d must be a multiple of 32{f', at most {max_d}' if max_d else ''}, got {d}")
    if problems * imgs * t > 2 ** 31 - 1:
        raise ValueError(f"{op}: problems * imgs * t exceeds 2^31 - 1")
    if x.dtype != torch.bfloat16 and not keep_fp32:
        x = x.to(torch.bfloat16)  # (fp32: rounded once)
    per16 = 8 if x.dtype == torch.bfloat16 else 4  # elements of a 16-byte chunk
    ok = x.stride(3) == 1 and (t == 1 or (x.stride(2) >= d and x.stride(2) % per16 == 0)) and \
        (imgs == 1 or (x.stride(1) >= 0 and x.stride(1) % per16 == 0)) and \
        (problems == 1 or (x.stride(0) >= 0 and x.stride(0) % per16 == 0)) and x.data_ptr() % 16 == 0
    if not ok:
        if refuse_strided_channels and x.stride(3) != 1:
            raise ValueError(f"{op}: the channels of {name} must be contiguous")
        x = x.contiguous()
    return DescOperand(x, x.stride(2) if t > 1 else d, x.stride(1) if imgs > 1 else 0, x.stride(0) if problems > 1 else 0,
                       problems, imgs, t, d)


def nn_cosine(x: torch.Tensor, y: torch.Tensor, mutual: bool = True):
    """Cosine nearest neighbours between descriptor maps (vdr_op_nn_cosine): x [P, tx, d], y [P, ty, d] on the device, bf16
    -- contiguous, or views with contiguous channels (column slices of a wider buffer, rows behind a prefix, a batch stride
    of 0 from expand(): one map against many), read in place.  fp32 inputs are rounded once to bf16 first.  d must be a
    multiple of 32.  Returns (row_sim [P, tx] fp32, row_idx [P, tx] int32, col_sim [P, ty], col_idx [P, ty]):
    row_sim[p, i] = max_j cos(x[p, i], y[p, j]) and row_idx the lowest j attaining it, col_* the same over i for every j;
    col_sim and col_idx are None when mutual=False (the column side is then not computed).  The [tx, ty] similarity matrix
    is never materialised.  The exact arithmetic is stated in include/vdr.h."""
    ox = desc_operand(x, "nn_cosine", "x", refuse_strided_channels=True)
    oy = desc_operand(y, "nn_cosine", "y", refuse_strided_channels=True)
    if ox.x.device != oy.x.device:
        raise ValueError("nn_cosine: x and y must be on the same device")
    if ox.problems != oy.problems or ox.d != oy.d:
        raise ValueError(f"nn_cosine: x {tuple(x.shape)} and y {tuple(y.shape)} must agree in P and d")
    P, tx, ty, d = ox.problems, ox.t, oy.t, ox.d
    lib = L.load()
    dev = x.device
    work = torch.empty((lib.vdr_nn_cosine_work_bytes(P, tx, ty),), dtype=torch.uint8, device=dev)
    row_sim = torch.empty((P, tx), dtype=torch.float32, device=dev)
    row_idx = torch.empty((P, tx), dtype=torch.int32, device=dev)
    col_sim = torch.empty((P, ty), dtype=torch.float32, device=dev) if mutual else None
    col_idx = torch.empty((P, ty), dtype=torch.int32, device=dev) if mutual else None
    L.check(lib.vdr_op_nn_cosine(ox.x.data_ptr(), ox.ld, ox.stride, tx, oy.x.data_ptr(), oy.ld, oy.stride, ty, P, d, work.data_ptr(),
                                 row_sim.data_ptr(), row_idx.data_ptr(), _p(col_sim), _p(col_idx), _s(ox.x)))
    return row_sim, row_idx, col_sim, col_idx


KNN_MAX_K = 16  # VDR_KNN_MAX_K (include/vdr.h)
KNN_METRICS = ("cosine", "l2")  # VDR_KNN_COSINE, VDR_KNN_L2


def check_knn(op: str, k, metric: str, tc: int, exclude_diag: bool) -> int:
    """The one wording of "no such neighbour list" (ValueError); returns k as an int."""
    if metric not in KNN_METRICS:
        raise ValueError(f"{op}: metric must be one of {KNN_METRICS}, got {metric!r}")
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError(f"{op}: k must be a positive integer, got {k!r}")
    if int(k) > KNN_MAX_K:
        raise ValueError(f"{op}: k must be at most {KNN_MAX_K}, got {k} (longer lists, such as DINO's 20 / 200, are out of scope)")
    if tc - int(bool(exclude_diag)) < int(k):
        raise ValueError(f"{op}: {tc} candidates{' without the own row' if exclude_diag else ''} are fewer than k = {k}")
    return int(k)


def knn(x: torch.Tensor, y: torch.Tensor, k: int, metric: str = "cosine", exclude_diag: bool = False):
    """The k nearest candidates of every query over ALL candidates (vdr_op_knn): x [P, tq, d] the queries, y [P, tc, d] the
    candidates; operands as nn_cosine takes them (bf16 read in place through views with contiguous channels, a batch stride
    of 0 from expand() -- many query sets against one bank --, fp32 rounded once to bf16; d a multiple of 32).  Returns
    (val [P, tq, k] fp32, idx [P, tq, k] int32), best first: metric="cosine" the cosine similarity with nn_cosine's bits,
    greater is better; metric="l2" the SQUARED distance, smaller is better; equal values in ascending index order.
    exclude_diag=True: candidate i is not eligible for query i (the k-NN graph of a map against itself).  k is 1..16 and at
    most the number of eligible candidates, so exactly k real neighbours come back.  The [tq, tc] score matrix is never
    materialised.  The exact arithmetic is stated in include/vdr.h."""
    ox = desc_operand(x, "knn", "x", refuse_strided_channels=True)
    oy = desc_operand(y, "knn", "y", refuse_strided_channels=True)
    if ox.x.device != oy.x.device:
        raise ValueError("knn: x and y must be on the same device")
    if ox.problems != oy.problems or ox.d != oy.d:
        raise ValueError(f"knn: x {tuple(x.shape)} and y {tuple(y.shape)} must agree in P and d")
    P, tq, tc, d = ox.problems, ox.t, oy.t, ox.d
    k = check_knn("knn", k, metric, tc, exclude_diag)
    if P * tq * k > 2 ** 31 - 1:
        raise ValueError("knn: P * tq * k exceeds 2^31 - 1")
    lib = L.load()
    dev = ox.x.device
    work = torch.empty((lib.vdr_knn_work_bytes(P, tq, tc, k),), dtype=torch.uint8, device=dev)
    val = torch.empty((P, tq, k), dtype=torch.float32, device=dev)
    idx = torch.empty((P, tq, k), dtype=torch.int32, device=dev)
    L.check(lib.vdr_op_knn(ox.x.data_ptr(), ox.ld, ox.stride, tq, oy.x.data_ptr(), oy.ld, oy.stride, tc, P, d, k,
                           KNN_METRICS.index(metric), int(bool(exclude_diag)), work.data_ptr(), val.data_ptr(), idx.data_ptr(), _s(ox.x)))
    return val, idx


LOCAL_CORR_MAX_RADIUS = 8  # VDR_LOCAL_CORR_MAX_RADIUS (include/vdr.h)


def check_local_radius(op: str, radius) -> int:
    """The one wording of "no such window" (ValueError); returns the radius as an int."""
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= LOCAL_CORR_MAX_RADIUS:
        raise ValueError(f"{op}: radius must be an integer in 1..{LOCAL_CORR_MAX_RADIUS}, got {radius!r}")
    return int(radius)


def local_correlation(x: torch.Tensor, y: torch.Tensor, grid, radius: int, cost: bool = True, best: bool = True,
                      transposed: bool = False):
    """Windowed correlation of two descriptor maps on one grid (vdr_op_local_correlation): x [P, t, d] the queries, y
    [P, t, d] the candidates, t = gh * gw for grid = (gh, gw); operands as nn_cosine takes them (bf16 read in place through
    views with contiguous channels, a batch stride of 0 from expand(), fp32 rounded once to bf16; d a multiple of 32).
    Every patch is compared with the patches at most `radius` (1..8) grid steps away in y and in x, W = 2 * radius + 1:
    returns (cost [P, t, W * W] fp32, best_sim [P, t] fp32, best_idx [P, t] int32).  Slot (dy + radius) * W + (dx + radius)
    of cost[p, i] is the cosine of x[p, i] and the candidate at displacement (dy, dx) -- vdr.local.offsets(radius) lists
    them --, -inf where that falls outside the grid; best_sim is the maximum over the window and best_idx the lowest
    candidate index that attains it.  cost=False / best=False skip that output (None in its place); one of them must be
    asked for.  The similarities have nn_cosine's bits; transposed=True multiplies by the candidate's norm first, which gives
    the reverse direction of a match -- local_correlation(y, x, transposed=True) beside local_correlation(x, y) -- the bits
    of nn_cosine(x, y)'s column side.  The exact arithmetic is stated in include/vdr.h."""
    ox = desc_operand(x, "local_correlation", "x", refuse_strided_channels=True)
    oy = desc_operand(y, "local_correlation", "y", refuse_strided_channels=True)
    if ox.x.device != oy.x.device:
        raise ValueError("local_correlation: x and y must be on the same device")
    if ox.problems != oy.problems or ox.d != oy.d or ox.t != oy.t:
        raise ValueError(f"local_correlation: x {tuple(x.shape)} and y {tuple(y.shape)} must agree in P, t and d")
    gh, gw = (int(v) for v in grid)
    if gh <= 0 or gw <= 0 or gh * gw != ox.t:
        raise ValueError(f"local_correlation: x has {ox.t} rows, the grid {gh} x {gw}")
    r = check_local_radius("local_correlation", radius)
    if not cost and not best:
        raise ValueError("local_correlation: no output asked for (cost=False and best=False)")
    P, t, d, WW = ox.problems, ox.t, ox.d, (2 * r + 1) ** 2
    if P * t * WW > 2 ** 31 - 1:
        raise ValueError("local_correlation: P * t * (2 radius + 1)^2 exceeds 2^31 - 1")
    lib = L.load()
    dev = ox.x.device
    work = torch.empty((lib.vdr_local_correlation_work_bytes(P, gh, gw, r),), dtype=torch.uint8, device=dev)
    c = torch.empty((P, t, WW), dtype=torch.float32, device=dev) if cost else None
    best_sim = torch.empty((P, t), dtype=torch.float32, device=dev) if best else None
    best_idx = torch.empty((P, t), dtype=torch.int32, device=dev) if best else None
    L.check(lib.vdr_op_local_correlation(ox.x.data_ptr(), ox.ld, ox.stride, oy.x.data_ptr(), oy.ld, oy.stride, P, gh, gw, d, r,
                                         int(bool(transposed)), work.data_ptr(), _p(c), _p(best_sim), _p(best_idx), _s(ox.x)))
    return c, best_sim, best_idx


WINDOW_VOTE_MAX_SOURCES, WINDOW_VOTE_MAX_K, WINDOW_VOTE_MAX_CLASSES = 8, 16, 64  # VDR_WINDOW_VOTE_MAX_* (include/vdr.h)
VOTE_WEIGHTS = ("softmax", "uniform")  # VDR_VOTE_SOFTMAX, VDR_VOTE_UNIFORM


def check_window_vote(op: str, cost, src, grid, k, weights, temperature):
    """The refusals of the window vote (ValueError), shared by vdr.ops.window_vote and its torch statement
    vdr.local.vote_window -- vdr_op_window_vote's, in its order.  Returns (P, S, gh, gw, radius, k, C)."""
    if not isinstance(cost, torch.Tensor) or cost.dim() != 4 or cost.dtype != torch.float32:
        raise ValueError(f"{op}: cost must be a [P, S, t, W * W] float32 tensor")
    if not isinstance(src, torch.Tensor) or src.dim() != 4 or src.dtype != torch.float32:
        raise ValueError(f"{op}: src must be a [P, S, t, C] float32 tensor")
    if cost.device != src.device:
        raise ValueError(f"{op}: cost and src must be on the same device")
    if tuple(cost.shape[:3]) != tuple(src.shape[:3]):
        raise ValueError(f"{op}: cost {tuple(cost.shape)} and src {tuple(src.shape)} must agree in P, S and t")
    P, S, t, WW = (int(v) for v in cost.shape)
    C = int(src.shape[3])
    gh, gw = (int(v) for v in grid)
    if min(P, S, gh, gw, C) <= 0:
        raise ValueError(f"{op}: problems, sources, gh, gw and n_classes must be positive")
    if gh * gw != t:
        raise ValueError(f"{op}: cost has {t} rows, the grid {gh} x {gw}")
    if P * S * t > 2 ** 31 - 1:
        raise ValueError(f"{op}: problems * sources * gh * gw exceeds 2^31 - 1")
    if S > WINDOW_VOTE_MAX_SOURCES:
        raise ValueError(f"{op}: sources must be 1 .. {WINDOW_VOTE_MAX_SOURCES}, got {S}")
    r = next((r for r in range(1, LOCAL_CORR_MAX_RADIUS + 1) if (2 * r + 1) ** 2 == WW), None)
    if r is None:
        raise ValueError(f"{op}: cost has {WW} slots, which is (2 r + 1)^2 for no radius in 1..{LOCAL_CORR_MAX_RADIUS}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= WINDOW_VOTE_MAX_K:
        raise ValueError(f"{op}: k must be an integer in 1 .. {WINDOW_VOTE_MAX_K}, got {k!r}")
    if C > WINDOW_VOTE_MAX_CLASSES:
        raise ValueError(f"{op}: n_classes must be 1 .. {WINDOW_VOTE_MAX_CLASSES}, got {C}")
    corner = S * min(gh, r + 1) * min(gw, r + 1)
    if int(k) > corner:
        raise ValueError(f"{op}: k exceeds the {corner} in-grid candidates of a corner patch, sources * min(gh, radius + 1) * "
                         f"min(gw, radius + 1), got {k}")
    if weights not in VOTE_WEIGHTS:
        raise ValueError(f"{op}: weights must be one of {VOTE_WEIGHTS}, got {weights!r}")
    T = torch.tensor(float(temperature), dtype=torch.float32)  # (what the op sees: the fp32 value)
    if not float(T) > 0 or not bool(torch.isfinite(T)):
        raise ValueError(f"{op}: temperature must be positive and finite, got {temperature!r}")
    if P * S * t * max(WW, C) > 2 ** 31 - 1:
        raise ValueError(f"{op}: an element count (cost or src) exceeds 2^31 - 1")
    return P, S, gh, gw, r, int(k), C


def window_vote(cost: torch.Tensor, src: torch.Tensor, grid, k: int, weights: str = "softmax", temperature: float = 0.1,
                labels: bool = True, neighbours: bool = True):
    """The multi-source soft window vote (vdr_op_window_vote): cost [P, S, t, W * W] fp32 -- per problem the S cost volumes of
    one target map against S source maps on grid = (gh, gw), as local_correlation writes them (one call with the target
    expand()ed over the S sources gives a problem's block) --, src [P, S, t, C] fp32 the sources' class scores (finite,
    non-negative; one-hot rows are hard labels).  Every patch takes the k best candidates inside the grid over all S windows
    -- greater value first, then lower source, then lower slot -- and votes their src rows with weights
    exp((v_m - v_0) / temperature) ("softmax") or 1 ("uniform"), normalised.  Returns (scores [P, t, C] fp32, labels [P, t]
    int32: the lowest class of the largest score, idx [P, t, k] int32: s * t + j of the neighbours, best first, val [P, t, k]
    fp32: their values); labels=False / neighbours=False skip those outputs (None in their place).  The radius is the one
    whose (2 r + 1)^2 is cost's last dimension.  S <= 8, k <= 16 and at most the in-grid candidates of a corner patch, C <= 64.
    vdr.local.vote_window is the same in plain torch; the exact arithmetic is stated in include/vdr.h."""
    P, S, gh, gw, r, k, C = check_window_vote("window_vote", cost, src, grid, k, weights, temperature)
    if cost.device.type != "cuda":
        raise ValueError("window_vote: cost and src must be on the device (vdr.local.vote_window runs on any)")
    cost, src = cost.contiguous(), src.contiguous()
    lib = L.load()
    dev, t = cost.device, gh * gw
    scores = torch.empty((P, t, C), dtype=torch.float32, device=dev)
    lab = torch.empty((P, t), dtype=torch.int32, device=dev) if labels else None
    idx = torch.empty((P, t, k), dtype=torch.int32, device=dev) if neighbours else None
    val = torch.empty((P, t, k), dtype=torch.float32, device=dev) if neighbours else None
    L.check(lib.vdr_op_window_vote(cost.data_ptr(), src.data_ptr(), P, S, gh, gw, r, k, C, VOTE_WEIGHTS.index(weights),
                                   float(temperature), scores.data_ptr(), _p(lab), _p(idx), _p(val), _s(cost)))
    return scores, lab, idx, val


def bits_pitch(t: int) -> int:
    """int32 words per row of a bit-packed [t, t] graph: ceil(t / 32) rounded up to a multiple of 4 (16-byte rows)"""
    return (int(t) + 127) // 128 * 4


def affinity_bits(x: torch.Tensor, tau: float = 0.2, exclude_diag: bool = False) -> torch.Tensor:
    """Thresholded affinity graph of descriptor maps (vdr_op_affinity_bits): x [P, t, d] on the device, bf16 -- contiguous, or
    a view with contiguous channels, read in place as nn_cosine reads its operands; fp32 is rounded once to bf16 first.  d
    must be a multiple of 32.  Returns bits [P, t, bits_pitch(t)] int32: bit (j & 31) of bits[p, i, j >> 5] is
    cos(x[p, i], x[p, j]) > tau (the diagonal cleared with exclude_diag); bits of columns >= t and the padding words are 0.
    The graph is symmetric bit for bit; the [t, t] matrix of scores is never materialised.  The exact arithmetic is stated in
    include/vdr.h."""
    o = desc_operand(x, "affinity_bits", refuse_strided_channels=True)
    x, P, t, d = o.x, o.problems, o.t, o.d
    tau = float(tau)
    if tau != tau:
        raise ValueError("affinity_bits: tau is NaN")
    lib = L.load()
    pitch = bits_pitch(t)
    work = torch.empty((lib.vdr_affinity_work_bytes(P, t),), dtype=torch.uint8, device=x.device)
    bits = torch.empty((P, t, pitch), dtype=torch.int32, device=x.device)
    L.check(lib.vdr_op_affinity_bits(x.data_ptr(), o.ld, o.stride, t, P, d, tau, int(bool(exclude_diag)), work.data_ptr(), bits.data_ptr(),
                                     pitch, _s(x)))
    return bits


def _check_bits(bits: torch.Tensor, op: str):
    if not isinstance(bits, torch.Tensor) or bits.dim() != 3 or bits.dtype != torch.int32:
        raise TypeError(f"{op}: bits must be a [P, t, pitch] int32 tensor")
    if bits.shape[0] <= 0 or bits.shape[1] <= 0 or bits.shape[2] != bits_pitch(bits.shape[1]):
        raise ValueError(f"{op}: bits {tuple(bits.shape)} is not [P, t, bits_pitch(t)]")


def bits_matvec(bits: torch.Tensor, v: torch.Tensor, degree: bool = False):
    """The product of a bit-packed graph with 1 .. 8 columns (vdr_op_bits_matvec): bits [P, t, pitch] int32 from
    affinity_bits, v [P, t, nv] (or [P, t]) fp32 -> y of v's shape, y[p, i, c] = sum over j with B[p, i, j] of v[p, j, c], in
    the fixed fp32 order stated in include/vdr.h.  degree=True returns (y, deg [P, t] int32), the exact row popcounts."""
    _check_bits(bits, "bits_matvec")
    if not bits.is_cuda:
        raise TypeError("bits_matvec: bits must live on the HIP device")
    P, t, pitch = bits.shape
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() not in (2, 3) or v.device != bits.device:
        raise TypeError("bits_matvec: v must be a [P, t, nv] or [P, t] float32 tensor on the device of bits")
    flat = v.dim() == 2
    v3 = v.unsqueeze(2) if flat else v
    if v3.shape[0] != P or v3.shape[1] != t or not 1 <= v3.shape[2] <= 8:
        raise ValueError(f"bits_matvec: v {tuple(v.shape)} does not match bits {tuple(bits.shape)} with 1 <= nv <= 8")
    nv = v3.shape[2]
    bits, v3 = bits.contiguous(), v3.contiguous()
    y = torch.empty((P, t, nv), dtype=torch.float32, device=bits.device)
    deg = torch.empty((P, t), dtype=torch.int32, device=bits.device) if degree else None
    L.check(L.load().vdr_op_bits_matvec(bits.data_ptr(), pitch, t, P, v3.data_ptr(), nv, y.data_ptr(), _p(deg), _s(bits)))
    y = y[:, :, 0] if flat else y
    return (y, deg) if degree else y


def pack_bits(b: torch.Tensor) -> torch.Tensor:
    """bool [P, t, t] -> bits [P, t, bits_pitch(t)] int32 in affinity_bits' layout.  Plain torch: for tests and small maps."""
    if b.dim() != 3 or b.shape[1] != b.shape[2]:
        raise ValueError(f"pack_bits: a [P, t, t] tensor expected, got {tuple(b.shape)}")
    P, t, _ = b.shape
    pitch = bits_pitch(t)
    full = torch.zeros((P, t, pitch * 32), dtype=torch.int64, device=b.device)
    full[:, :, :t] = b.to(torch.int64)
    words = (full.view(P, t, pitch, 32) << torch.arange(32, device=b.device, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def unpack_bits(bits: torch.Tensor, t: int) -> torch.Tensor:
    """bits [P, t, pitch] int32 -> bool [P, t, t], B[p, i, j] = bit (j & 31) of bits[p, i, j >> 5].  Plain torch, on the
    device of bits: for tests and small maps."""
    _check_bits(bits, "unpack_bits")
    if int(t) != bits.shape[1]:
        raise ValueError(f"unpack_bits: t = {t} but bits has {bits.shape[1]} rows")
    sh = torch.arange(32, device=bits.device, dtype=torch.int64)
    b = ((bits.to(torch.int64).unsqueeze(-1) >> sh) & 1).to(torch.bool)
    return b.reshape(bits.shape[0], bits.shape[1], -1)[:, :, :t]


def best_buddies(row_idx: torch.Tensor, col_idx: torch.Tensor) -> torch.Tensor:
    """Mutual nearest neighbours: row_idx [P, tx] (for every row of x its nearest row of y), col_idx [P, ty] (the reverse)
    -> bool [P, tx], col_idx[p, row_idx[p, i]] == i.  Pure torch; CPU tensors work too."""
    if row_idx.dim() != 2 or col_idx.dim() != 2 or row_idx.shape[0] != col_idx.shape[0]:
        raise ValueError(f"best_buddies: row_idx [P, tx] and col_idx [P, ty] expected, got {tuple(row_idx.shape)} and "
                         f"{tuple(col_idx.shape)}")
    back = torch.gather(col_idx.long(), 1, row_idx.long())
    return back == torch.arange(row_idx.shape[1], device=row_idx.device).unsqueeze(0)


def _pca_operand(x, op: str, joint: bool):
    """a PCA operand: the input's dtype is kept, d <= 2048 -> (tensor, in_dtype, ld, image_stride, problems, imgs, t, d)"""
    o = desc_operand(x, op, joint=joint, keep_fp32=True, max_d=2048)
    return o.x, o.dtype, o.ld, o.stride, o.problems, o.imgs, o.t, o.d


def _pca_work(lib, problems, imgs, t, d, dev):
    return torch.empty((lib.vdr_pca_work_bytes(problems, imgs, t, d),), dtype=torch.uint8, device=dev)


def _pca_vector(v, name: str, op: str, shape, dev):
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != tuple(shape):
        raise ValueError(f"{op}: {name} must be a float32 tensor of shape {tuple(shape)}, got "
                         f"{tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    if v.device != dev:
        raise ValueError(f"{op}: {name} must be on x's device")
    return v.contiguous()


def col_mean(x: torch.Tensor, joint: bool = False) -> torch.Tensor:
    """Column means of descriptor maps (vdr_op_col_mean): x [P, t, d] bf16 / fp32 on the device -> [P, d] fp32, one mean
    per image, or [1, d] with joint=True (the P * t rows of all images as one problem).  fp32 sums in a fixed order, one
    IEEE division (include/vdr.h).  d must be a multiple of 32, at most 2048."""
    x, dt, ld, stride, problems, imgs, t, d = _pca_operand(x, "col_mean", joint)
    lib = L.load()
    work = _pca_work(lib, problems, imgs, t, d, x.device)
    mean = torch.empty((problems, d), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_col_mean(x.data_ptr(), dt, ld, stride, problems, imgs, t, d, work.data_ptr(), mean.data_ptr(), _s(x)))
    return mean


def covariance(x: torch.Tensor, mean=None, joint: bool = False):
    """Centred covariance of descriptor maps (vdr_op_covariance): x [P, t, d] bf16 / fp32 on the device -> (mean [P, d],
    cov [P, d, d]) fp32 -- [1, d] and [1, d, d] with joint=True.  mean=None: col_mean(x, joint); any other [problems, d]
    fp32 vector is taken as it is.  z = bf16(float(x) - mean), cov = z^T z / (R - 1) accumulated in fp32 by bf16 MFMAs in
    chunks of 1024 rows; exactly symmetric (include/vdr.h).  Needs R >= 2 rows per problem."""
    x, dt, ld, stride, problems, imgs, t, d = _pca_operand(x, "covariance", joint)
    if imgs * t < 2:
        raise ValueError("covariance: needs at least 2 rows per problem")
    lib = L.load()
    work = _pca_work(lib, problems, imgs, t, d, x.device)
    if mean is None:
        mean = torch.empty((problems, d), dtype=torch.float32, device=x.device)
        L.check(lib.vdr_op_col_mean(x.data_ptr(), dt, ld, stride, problems, imgs, t, d, work.data_ptr(), mean.data_ptr(), _s(x)))
    else:
        mean = _pca_vector(mean, "mean", "covariance", (problems, d), x.device)
    cov = torch.empty((problems, d, d), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_covariance(x.data_ptr(), dt, ld, stride, problems, imgs, t, d, mean.data_ptr(), work.data_ptr(),
                                  cov.data_ptr(), _s(x)))
    return mean, cov


def pca_project(x: torch.Tensor, mean: torch.Tensor, components: torch.Tensor, scale: bool = False):
    """Projection of descriptor maps on given components (vdr_op_pca_project): x [P, t, d] bf16 / fp32 on the device, mean
    [problems, d] and components [problems, k, d] fp32, k = 1..8; problems = P projects every image with its own mean and
    components, problems = 1 (with P > 1) all P * t rows with the one set (joint).  Returns (proj [problems, R, k] fp32,
    minmax [problems, 2] fp32), R = t or P * t: proj = (x - mean) . components^T in fp32, minmax the range of a
    problem's whole block; scale=True rescales proj to (proj - min) / (max - min) where max != min (include/vdr.h)."""
    if not isinstance(components, torch.Tensor) or components.dim() != 3:
        raise ValueError("pca_project: components must be a [problems, k, d] float32 tensor")
    problems, k = int(components.shape[0]), int(components.shape[1])
    if not 1 <= k <= 8:
        raise ValueError(f"pca_project: k must be 1..8, got {k}")
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise TypeError("pca_project: x must be a [P, t, d] float32 or bfloat16 tensor")
    if problems not in (1, x.shape[0]):
        raise ValueError(f"pca_project: {problems} sets of components for {x.shape[0]} images (one per image, or one for all)")
    x, dt, ld, stride, problems, imgs, t, d = _pca_operand(x, "pca_project", problems == 1 and x.shape[0] > 1)
    mean = _pca_vector(mean, "mean", "pca_project", (problems, d), x.device)
    components = _pca_vector(components, "components", "pca_project", (problems, k, d), x.device)
    lib = L.load()
    work = _pca_work(lib, problems, imgs, t, d, x.device)
    proj = torch.empty((problems, imgs * t, k), dtype=torch.float32, device=x.device)
    minmax = torch.empty((problems, 2), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_pca_project(x.data_ptr(), dt, ld, stride, problems, imgs, t, d, mean.data_ptr(), components.data_ptr(), k,
                                   int(bool(scale)), work.data_ptr(), proj.data_ptr(), minmax.data_ptr(), _s(x)))
    return proj, minmax


TOPK_TOL = 3.3e-7    # VDR_TOPK_TOL (include/vdr.h)
TOPK_MAX_ITER = 146  # VDR_TOPK_MAX_ITER


def _topk_operand(x, op: str):
    """an operand of the per-image Gram side: the input's dtype is kept, any d % 32 == 0 -> (tensor, in_dtype, ld, image_stride,
    problems, t, d)"""
    o = desc_operand(x, op, keep_fp32=True)
    return o.x, o.dtype, o.ld, o.stride, o.problems, o.t, o.d


def _topk_work(lib, problems, t, d, k, dev):
    return torch.empty((lib.vdr_pca_topk_work_bytes(problems, t, d, k),), dtype=torch.uint8, device=dev)


def col_mean_any(x: torch.Tensor) -> torch.Tensor:
    """col_mean per image at any width (vdr_op_col_mean_any): x [P, t, d] bf16 / fp32 on the device -> [P, d] fp32, bit for
    bit col_mean's result where d <= 2048."""
    x, dt, ld, stride, P, t, d = _topk_operand(x, "col_mean_any")
    lib = L.load()
    work = _topk_work(lib, P, t, d, 1, x.device)
    mean = torch.empty((P, d), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_col_mean_any(x.data_ptr(), dt, ld, stride, P, t, d, work.data_ptr(), mean.data_ptr(), _s(x)))
    return mean


def gram(x: torch.Tensor, mean=None):
    """Centred Gram matrices of descriptor maps (vdr_op_gram), the t x t side of the PCA for t < d: x [P, t, d] bf16 / fp32
    on the device -> (mean [P, d], gram [P, t, t]) fp32, per image.  mean=None: col_mean_any(x); any other [P, d] fp32 vector is
    taken as it is.  z = bf16(float(x) - mean), gram = z z^T / (t - 1) accumulated in fp32 by bf16 MFMAs in chunks of 256
    columns; exactly symmetric (include/vdr.h).  d % 32 == 0 with no upper bound, 2 <= t <= 4096."""
    x, dt, ld, stride, P, t, d = _topk_operand(x, "gram")
    if not 2 <= t <= 4096:
        raise ValueError(f"gram: t must be 2..4096 rows per image, got {t}")
    lib = L.load()
    work = _topk_work(lib, P, t, d, 1, x.device)
    if mean is None:
        mean = torch.empty((P, d), dtype=torch.float32, device=x.device)
        L.check(lib.vdr_op_col_mean_any(x.data_ptr(), dt, ld, stride, P, t, d, work.data_ptr(), mean.data_ptr(), _s(x)))
    else:
        mean = _pca_vector(mean, "mean", "gram", (P, d), x.device)
    g = torch.empty((P, t, t), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_gram(x.data_ptr(), dt, ld, stride, P, t, d, mean.data_ptr(), work.data_ptr(), g.data_ptr(), _s(x)))
    return mean, g


def sym_topk(a: torch.Tensor, k: int, tol: float = TOPK_TOL, max_iter: int = TOPK_MAX_ITER):
    """The k largest eigenpairs of symmetric positive semi-definite matrices (vdr_op_sym_topk): a [P, n, n] fp32 on the
    device, n = 2..4096, k = 1..min(8, n) -> (values [P, k] fp32 descending, vectors [P, k, n] fp32 of unit length with the
    entry of largest magnitude positive, iters [P] int32, resid [P] fp32).  Block subspace iteration with a Rayleigh-Ritz
    step on 16 columns, all on the device, no host synchronisation; a problem is done when its k leading residuals are at or
    below tol * theta_1.  resid > tol tells a problem that ran into max_iter (include/vdr.h)."""
    if not isinstance(a, torch.Tensor) or a.dim() != 3 or a.shape[1] != a.shape[2] or a.dtype != torch.float32:
        raise TypeError("sym_topk: a must be a [P, n, n] float32 tensor")
    if not a.is_cuda:
        raise TypeError("sym_topk: a must live on the HIP device")
    P, n = int(a.shape[0]), int(a.shape[1])
    if P <= 0:
        raise ValueError("sym_topk: empty operand")
    if not 2 <= n <= 4096:
        raise ValueError(f"sym_topk: n must be 2..4096, got {n}")
    k = int(k)
    if not 1 <= k <= min(8, n):
        raise ValueError(f"sym_topk: k must be 1..min(8, n) = 1..{min(8, n)}, got {k}")
    if not float(tol) >= 0.0 or int(max_iter) < 1:
        raise ValueError(f"sym_topk: tol must be >= 0 and max_iter >= 1, got {tol} and {max_iter}")
    a = a.contiguous()
    lib = L.load()
    work = _topk_work(lib, P, n, 32, 1, a.device)
    values = torch.empty((P, k), dtype=torch.float32, device=a.device)
    vectors = torch.empty((P, k, n), dtype=torch.float32, device=a.device)
    iters = torch.empty((P,), dtype=torch.int32, device=a.device)
    resid = torch.empty((P,), dtype=torch.float32, device=a.device)
    L.check(lib.vdr_op_sym_topk(a.data_ptr(), P, n, k, float(tol), int(max_iter), work.data_ptr(), values.data_ptr(),
                                vectors.data_ptr(), iters.data_ptr(), resid.data_ptr(), _s(a)))
    return values, vectors, iters, resid


def pca_back_project(x: torch.Tensor, mean: torch.Tensor, u: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """From eigenvectors of the Gram matrix to principal components (vdr_op_pca_back_project): x [P, t, d] bf16 / fp32 on the
    device, mean [P, d], u [P, k, t], values [P, k] fp32 -> components [P, k, d] fp32,
    c[p, j] = sum_r u[p, j, r] * (float(x[r]) - mean[p]) in fp32 in col_mean's row order, divided by its float64 norm; a
    component with values[p, j] <= 0 comes back as zeros (include/vdr.h).  k = 1..8, any d % 32 == 0."""
    if not isinstance(u, torch.Tensor) or u.dim() != 3:
        raise ValueError("pca_back_project: u must be a [P, k, t] float32 tensor")
    k = int(u.shape[1])
    if not 1 <= k <= 8:
        raise ValueError(f"pca_back_project: k must be 1..8, got {k}")
    x, dt, ld, stride, P, t, d = _topk_operand(x, "pca_back_project")
    mean = _pca_vector(mean, "mean", "pca_back_project", (P, d), x.device)
    u = _pca_vector(u, "u", "pca_back_project", (P, k, t), x.device)
    values = _pca_vector(values, "values", "pca_back_project", (P, k), x.device)
    lib = L.load()
    work = _topk_work(lib, P, t, d, k, x.device)
    comps = torch.empty((P, k, d), dtype=torch.float32, device=x.device)
    L.check(lib.vdr_op_pca_back_project(x.data_ptr(), dt, ld, stride, P, t, d, mean.data_ptr(), u.data_ptr(), values.data_ptr(), k,
                                        work.data_ptr(), comps.data_ptr(), _s(x)))
    return comps


KMEANS_CHUNK = 256  # VDR_KMEANS_CHUNK (include/vdr.h)
KMEANS_MAX_K = 1024


KmeansOperand = DescOperand  # (the name the k-means family and its callers know it by)


def kmeans_operand(x, joint: bool = False, op: str = "kmeans") -> DescOperand:
    """The operand of the k-means ops and of mahalanobis: desc_operand with x [problems, imgs, t, d] taken as it says (an
    expand()ed leading dimension, stride 0, is one map under many sets of centroids) and fp32 rounded once to bf16."""
    return desc_operand(x, op, joint=joint, four_d=True)


def _kmeans_k(o: KmeansOperand, centroids, op: str) -> int:
    if not isinstance(centroids, torch.Tensor) or centroids.dim() != 3 or centroids.dtype != torch.float32 or \
            centroids.shape[0] != o.problems or centroids.shape[2] != o.d:
        raise ValueError(f"{op}: centroids must be a float32 tensor of shape ({o.problems}, k, {o.d}), got "
                         f"{tuple(centroids.shape) if isinstance(centroids, torch.Tensor) else type(centroids).__name__}")
    if centroids.device != o.x.device or not centroids.is_contiguous():
        raise ValueError(f"{op}: centroids must be contiguous and on x's device")
    k = int(centroids.shape[1])
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError(f"{op}: k must be 1..{KMEANS_MAX_K}, got {k}")
    if k > o.R:
        raise ValueError(f"{op}: k = {k} exceeds the {o.R} rows of a problem")
    return k


def _kmeans_ints(v, name: str, op: str, shape, dev):
    if not isinstance(v, torch.Tensor) or v.dtype != torch.int32 or tuple(v.shape) != tuple(shape) or v.device != dev or \
            not v.is_contiguous():
        raise ValueError(f"{op}: {name} must be a contiguous int32 tensor of shape {tuple(shape)} on x's device")
    return v


def kmeans_assign(x, centroids: torch.Tensor, labels=None, joint: bool = False, active=None, out=None, work=None):
    """The assignment step of Lloyd's k-means (vdr_op_kmeans_assign): x as kmeans_operand takes it, centroids [problems, k, d]
    fp32.  Returns (labels [problems, R] int32, min_dist [problems, R] fp32, inertia [problems] fp32, changed [problems]
    int32): the nearest centroid of every row by h = cc - 2 x.c with the centroid split into two bf16 operands, the lowest
    index on a tie; changed counts the rows whose label differs from the one passed in `labels` (None: every row counts;
    a given tensor is updated in place and returned).  active [problems] int32: problems whose flag is 0 are left
    untouched.  out: (min_dist, inertia, changed) to write into.  The R x k matrix is never materialised; the exact
    arithmetic is stated in include/vdr.h."""
    o = kmeans_operand(x, joint, "kmeans_assign")
    k = _kmeans_k(o, centroids, "kmeans_assign")
    dev = o.x.device
    if labels is None:
        labels = torch.full((o.problems, o.R), -1, dtype=torch.int32, device=dev)
    else:
        _kmeans_ints(labels, "labels", "kmeans_assign", (o.problems, o.R), dev)
    if active is not None:
        _kmeans_ints(active, "active", "kmeans_assign", (o.problems,), dev)
    if out is None:
        min_dist = torch.empty((o.problems, o.R), dtype=torch.float32, device=dev)
        inertia = torch.empty((o.problems,), dtype=torch.float32, device=dev)
        changed = torch.empty((o.problems,), dtype=torch.int32, device=dev)
    else:
        min_dist, inertia, changed = out
    lib = L.load()
    if work is None:
        work = o.work(k)
    L.check(lib.vdr_op_kmeans_assign(o.x.data_ptr(), o.ld, o.image_stride, o.problem_stride, o.problems, o.imgs, o.t, o.d, k,
                                     centroids.data_ptr(), _p(active), work.data_ptr(), labels.data_ptr(), min_dist.data_ptr(),
                                     inertia.data_ptr(), changed.data_ptr(), _s(o.x)))
    return labels, min_dist, inertia, changed


def kmeans_update(x, labels: torch.Tensor, centroids: torch.Tensor, joint: bool = False, active=None, inplace: bool = False,
                  counts=None, work=None):
    """The update step of Lloyd's k-means (vdr_op_kmeans_update): x as kmeans_operand takes it, labels [problems, R] int32,
    centroids [problems, k, d] fp32 (the previous ones).  Returns (centroids, counts [problems, k] int32): every centroid
    the fp32 sum of its rows -- bf16 MFMAs against a one-hot operand built on chip, in chunks of 256 rows -- divided once
    by its count; an empty cluster keeps its previous centroid's bits.  inplace=True writes into `centroids` itself.
    active [problems] int32: problems whose flag is 0 are left untouched (include/vdr.h)."""
    o = kmeans_operand(x, joint, "kmeans_update")
    k = _kmeans_k(o, centroids, "kmeans_update")
    dev = o.x.device
    _kmeans_ints(labels, "labels", "kmeans_update", (o.problems, o.R), dev)
    if active is not None:
        _kmeans_ints(active, "active", "kmeans_update", (o.problems,), dev)
    if not inplace:
        centroids = centroids.clone()
    if counts is None:
        counts = torch.zeros((o.problems, k), dtype=torch.int32, device=dev)
    lib = L.load()
    if work is None:
        work = o.work(k)
    L.check(lib.vdr_op_kmeans_update(o.x.data_ptr(), o.ld, o.image_stride, o.problem_stride, o.problems, o.imgs, o.t, o.d, k,
                                     labels.data_ptr(), _p(active), work.data_ptr(), centroids.data_ptr(), counts.data_ptr(),
                                     _s(o.x)))
    return centroids, counts


MAHALANOBIS_MAX_K = 2048  # VDR_MAHALANOBIS_MAX_K (include/vdr.h)


def _mahalanobis_model(v, name: str, inner, problems: int, dev):
    """A model tensor [problems, *inner] fp32 whose inner block is contiguous; its problem stride in elements (0 for an
    expand()ed leading dimension: one model under every problem)."""
    shape = (problems,) + tuple(inner)
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != shape:
        raise ValueError(f"mahalanobis: {name} must be a float32 tensor of shape {shape}, got "
                         f"{tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    if v.device != dev:
        raise ValueError(f"mahalanobis: {name} must be on x's device")
    n = 1
    for s in inner:
        n *= s
    stride = v.stride(0) if problems > 1 else n
    if not v[0].is_contiguous() or (stride != 0 and stride < n) or stride % 4 or v.data_ptr() % 16:
        v = v.contiguous()
        stride = n
    return v, stride


def mahalanobis(x, mean: torch.Tensor, whiten: torch.Tensor, joint: bool = False, out=None) -> torch.Tensor:
    """Squared Mahalanobis distances of descriptor rows (vdr_op_mahalanobis): x as kmeans_operand takes it ([P, t, d], one
    problem per image or joint=True; or [problems, imgs, t, d]; bf16 read in place, fp32 rounded once to bf16), mean
    [problems, d] fp32, whiten [problems, k, d] fp32 with contiguous [k, d] blocks, 1 <= k <= 2048 -- an expand()ed leading
    dimension (stride 0) is one model under every problem.  Returns d2 [problems, R] fp32, d2_i = sum_j (w_j . (x_i - mean))^2:
    the centred row and the whitening rows are each split into two bf16 operands, three of the four products are taken, and the
    squares are summed in one fixed order; the R x k matrix is never materialised.  out: a [problems, R] fp32 tensor with
    contiguous rows to write into.  The exact arithmetic is stated in include/vdr.h."""
    o = kmeans_operand(x, joint, "mahalanobis")
    dev = o.x.device
    if not isinstance(whiten, torch.Tensor) or whiten.dim() != 3:
        raise ValueError(f"mahalanobis: whiten must be a float32 tensor of shape ({o.problems}, k, {o.d})")
    k = int(whiten.shape[1])
    if not 1 <= k <= MAHALANOBIS_MAX_K:
        raise ValueError(f"mahalanobis: k must be 1..{MAHALANOBIS_MAX_K}, got {k}")
    mean, ms = _mahalanobis_model(mean, "mean", (o.d,), o.problems, dev)
    whiten, ws = _mahalanobis_model(whiten, "whiten", (k, o.d), o.problems, dev)
    if out is None:
        out = torch.empty((o.problems, o.R), dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (o.problems, o.R) or \
            out.device != dev or not out.is_contiguous():
        raise ValueError(f"mahalanobis: out must be a contiguous float32 tensor of shape ({o.problems}, {o.R}) on x's device")
    lib = L.load()
    L.check(lib.vdr_op_mahalanobis(o.x.data_ptr(), o.ld, o.image_stride, o.problem_stride, o.problems, o.imgs, o.t, o.d,
                                   mean.data_ptr(), ms, whiten.data_ptr(), ws, k, out.data_ptr(), _s(o.x)))
    return out


UPSAMPLE_MAX_RADIUS = 3
UPSAMPLE_MAX_GUIDE_CHANNELS = 4


def _dt(t):
    return L.VDR_BF16 if t.dtype == torch.bfloat16 else L.VDR_F32


def _upsample_guide(guide, patch, stride, op: str):
    """(B, Cg, H, W, p, s, gh, gw) of a guide batch under a patch grid, or the ValueError / TypeError of a bad one"""
    if not isinstance(guide, torch.Tensor) or guide.dim() != 4 or guide.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{op}: guide must be a [B, Cg, H, W] float32 or bfloat16 tensor")
    p, s = int(patch), int(stride)
    if p <= 0 or s <= 0 or p % s:
        raise ValueError(f"{op}: stride must be positive and divide patch, got patch {patch}, stride {stride}")
    B, Cg, H, W = guide.shape
    if B <= 0:
        raise ValueError(f"{op}: empty batch")
    if not 1 <= Cg <= UPSAMPLE_MAX_GUIDE_CHANNELS:
        raise ValueError(f"{op}: the guide must have 1..{UPSAMPLE_MAX_GUIDE_CHANNELS} channels, got {Cg}")
    if H < p or W < p or (H - p) % s or (W - p) % s:
        raise ValueError(f"{op}: a {H} x {W} guide is no patch + (g - 1) * stride grid of patch {p}, stride {s}")
    return B, Cg, H, W, p, s, (H - p) // s + 1, (W - p) // s + 1


def upsample_coefficients(stride: int, sigma_spatial: float, sigma_range: float):
    """(cs, cr) = (1 / (2 sigma_s^2 s^2), 1 / (2 sigma_r^2)) in double; sigma = inf gives 0.  The op rounds them once to fp32."""
    ss, sr = float(sigma_spatial), float(sigma_range)
    if not ss > 0.0 or not sr > 0.0:  # (NaN fails both)
        raise ValueError(f"upsample_guided: sigma_spatial and sigma_range must be > 0 (inf allowed), got {sigma_spatial}, {sigma_range}")
    cs = 0.0 if ss == float("inf") else 1.0 / (2.0 * ss * ss * float(stride) * float(stride))
    cr = 0.0 if sr == float("inf") else 1.0 / (2.0 * sr * sr)
    if cs > 3.0e38 or cr > 3.0e38:
        raise ValueError("upsample_guided: a sigma so small that its coefficient overflows fp32")
    return cs, cr


def guide_lowres(guide: torch.Tensor, patch: int, stride: int) -> torch.Tensor:
    """The low-resolution guide of upsample_guided alone (vdr_op_guide_lowres): guide [B, Cg, H, W] fp32 or bf16 -> [B, Cg, gh,
    gw] fp32, the mean of the guide over each patch's p x p footprint (fp32 sum in ascending (ky, kx), one IEEE division)."""
    B, Cg, H, W, p, s, gh, gw = _upsample_guide(guide, patch, stride, "guide_lowres")
    if not guide.is_cuda:
        raise TypeError("guide_lowres: guide must live on the HIP device")
    lib = L.load()
    guide = guide.contiguous()
    work = torch.empty((lib.vdr_upsample_work_bytes(B, Cg, gh, gw) // 4,), dtype=torch.float32, device=guide.device)
    L.check(lib.vdr_op_guide_lowres(guide.data_ptr(), _dt(guide), B, Cg, H, W, p, s, work.data_ptr(), _s(guide)))
    return work[:B * Cg * gh * gw].view(B, Cg, gh, gw)


def upsample_guided(features: torch.Tensor, guide: torch.Tensor, patch: int, stride: int, radius: int = 2,
                    sigma_spatial: float = 1.0, sigma_range: float = 0.1, confidence=None, box=None, out_dtype=None, out=None,
                    work=None) -> torch.Tensor:
    """Joint bilateral upsampling of a descriptor map to pixel resolution (vdr_op_upsample_guided): features [B, gh, gw, C]
    bf16 or fp32 (rounded once to bf16) -- contiguous, or a view with contiguous channels whose patch rows are evenly spaced
    (the key columns of a qkv activation: read in place) --, guide [B, Cg, H, W] fp32 or bf16, the image batch the features
    came from, H = patch + (gh - 1) * stride.  sigma_spatial is in patch-grid units (strides), sigma_range in guide units;
    confidence [B, gh, gw] fp32 >= 0 scales each patch's weight.  box = (y0, x0, y1, x1), half-open, in pixels (None: the
    whole image).  Returns [B, y1 - y0, x1 - x0, C] in out_dtype (default: the features' dtype); a box's output equals that
    region of the full output bit for bit.  The exact arithmetic is stated in include/vdr.h."""
    op = "upsample_guided"
    if not isinstance(features, torch.Tensor) or features.dim() != 4 or features.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{op}: features must be a [B, gh, gw, C] float32 or bfloat16 tensor")
    B, Cg, H, W, p, s, gh, gw = _upsample_guide(guide, patch, stride, op)
    if tuple(features.shape[:3]) != (B, gh, gw):
        raise ValueError(f"{op}: features {tuple(features.shape)} do not lie on the {B} x {gh} x {gw} grid of the guide")
    Cc = features.shape[3]
    if Cc <= 0 or Cc % 8:
        raise ValueError(f"{op}: C must be a positive multiple of 8, got {Cc}")
    r = int(radius)
    if not 1 <= r <= UPSAMPLE_MAX_RADIUS:
        raise ValueError(f"{op}: radius must be 1..{UPSAMPLE_MAX_RADIUS}, got {radius}")
    cs, cr = upsample_coefficients(s, sigma_spatial, sigma_range)
    if box is None:
        box = (0, 0, H, W)
    y0, x0, y1, x1 = (int(v) for v in box)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"{op}: box {tuple(box)} must be non-empty and inside the {H} x {W} image")
    if out_dtype is None:
        out_dtype = features.dtype
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    if confidence is not None and (not isinstance(confidence, torch.Tensor) or confidence.dtype != torch.float32 or
                                   tuple(confidence.shape) != (B, gh, gw)):
        raise ValueError(f"{op}: confidence must be a float32 tensor of shape ({B}, {gh}, {gw})")
    if Cc > 1 and features.stride(3) != 1:
        raise ValueError(f"{op}: the channels of features must be contiguous")
    if not features.is_cuda or not guide.is_cuda or (confidence is not None and not confidence.is_cuda):
        raise TypeError(f"{op}: features, guide and confidence must live on the HIP device")
    if guide.device != features.device or (confidence is not None and confidence.device != features.device):
        raise ValueError(f"{op}: features, guide and confidence must be on the same device")
    per16 = 8 if features.dtype == torch.bfloat16 else 4
    ld = features.stride(2) if gw > 1 else features.stride(1) if gh > 1 else Cc
    if gh > 1 and features.stride(1) != gw * ld:
        ld = -1  # (patch rows not evenly spaced: a copy)
    image_stride = features.stride(0) if B > 1 else 0
    if ld < Cc or ld % per16 or image_stride < 0 or image_stride % per16 or features.data_ptr() % 16:
        features = features.contiguous()
        ld, image_stride = Cc, gh * gw * Cc
    lib = L.load()
    dev = features.device
    guide = guide.contiguous()
    if confidence is not None:
        confidence = confidence.contiguous()
    shape = (B, y1 - y0, x1 - x0, Cc)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != out_dtype or tuple(out.shape) != shape or out.device != dev or \
            not out.is_contiguous():
        raise ValueError(f"{op}: out must be a contiguous {out_dtype} tensor of shape {shape} on the features' device")
    need = lib.vdr_upsample_work_bytes(B, Cg, gh, gw)
    if work is None:
        work = torch.empty((need // 4,), dtype=torch.float32, device=dev)
    elif not isinstance(work, torch.Tensor) or work.dtype != torch.float32 or work.device != dev or not work.is_contiguous() or \
            work.numel() * 4 < need:
        raise ValueError(f"{op}: work must be a contiguous float32 tensor of at least {need // 4} elements on the features' device")
    L.check(lib.vdr_op_upsample_guided(features.data_ptr(), _dt(features), ld, image_stride, B, gh, gw, Cc, guide.data_ptr(),
                                       _dt(guide), Cg, H, W, p, s, r, cs, cr, _p(confidence), y0, x0, y1, x1, work.data_ptr(),
                                       out.data_ptr(), _dt(out), _s(features)))
    return out


def patch_embed(images, weight, bias, p, pos=None, row_stride=None, row_offset=0, out=None):
    """images [B,C,H,H] fp32/bf16; weight [D,C,p,p] (any float dtype); returns bf16 [B*row_stride, D]."""
    lib = L.load()
    B, Cc, H, _ = images.shape
    D = weight.shape[0]
    g = H // p
    n = g * g
    K = Cc * p * p
    Kp = (K + 63) // 64 * 64
    Wp = torch.zeros((D, Kp), dtype=torch.bfloat16, device=images.device)
    Wp[:, :K] = weight.reshape(D, K).to(torch.bfloat16)
    col = torch.empty((B * n * Kp + 4096,), dtype=torch.bfloat16, device=images.device)
    row_stride = n if row_stride is None else row_stride
    if out is None:
        out = torch.zeros((B * row_stride, D), dtype=torch.bfloat16, device=images.device)
    images = images.contiguous()
    L.check(lib.vdr_op_patch_embed(images.data_ptr(), 1 if images.dtype == torch.bfloat16 else 0, Wp.data_ptr(),
                                   _p(bias), _p(pos), col.data_ptr(), out.data_ptr(), B, Cc, H, p, D, row_stride,
                                   row_offset, _s(images)))
    return out


def patch_embed_strided(images, weight, bias, p, stride, pos=None, row_stride=None, row_offset=0, return_col=False):
    """Conv2d(kernel=p, stride=stride) patch embedding (vdr_op_patch_embed_strided): images [B,C,H,W] fp32/bf16, (H - p) and
    (W - p) multiples of stride; weight [D,C,p,p]; returns bf16 [B*row_stride, D] (and, return_col, the col matrix
    [B*n, Kp] the GEMM read: written whenever stride < p)."""
    lib = L.load()
    B, Cc, H, W = images.shape
    D = weight.shape[0]
    n = ((H - p) // stride + 1) * ((W - p) // stride + 1)
    K = Cc * p * p
    Kp = (K + 63) // 64 * 64
    Wp = torch.zeros((D, Kp), dtype=torch.bfloat16, device=images.device)
    Wp[:, :K] = weight.reshape(D, K).to(torch.bfloat16)
    col = torch.full((B * n * Kp + 4096,), float("nan"), dtype=torch.bfloat16, device=images.device)
    row_stride = n if row_stride is None else row_stride
    out = torch.zeros((B * row_stride, D), dtype=torch.bfloat16, device=images.device)
    images = images.contiguous()
    L.check(lib.vdr_op_patch_embed_strided(images.data_ptr(), 1 if images.dtype == torch.bfloat16 else 0, Wp.data_ptr(),
                                           _p(bias), _p(pos), col.data_ptr(), out.data_ptr(), B, Cc, H, W, p, stride, D,
                                           row_stride, row_offset, _s(images)))
    return (out, col[:B * n * Kp].view(B * n, Kp)) if return_col else out


def interpolate_pos(pos: torch.Tensor, native_grid, grid) -> torch.Tensor:
    """pos [gh0*gw0, D] fp32 on the device (the patch rows of a position table, no CLS row) -> [gh*gw, D] fp32: DINOv2 /
    transformers interpolate_pos_encoding (vdr_op_interpolate_pos: bicubic, align_corners=False, fp64 arithmetic)."""
    lib = L.load()
    (gh0, gw0), (gh, gw) = native_grid, grid
    assert pos.is_cuda and pos.dtype == torch.float32 and pos.is_contiguous() and pos.dim() == 2
    assert pos.shape[0] == gh0 * gw0
    D = pos.shape[1]
    out = torch.empty((gh * gw, D), dtype=torch.float32, device=pos.device)
    L.check(lib.vdr_op_interpolate_pos(pos.data_ptr(), gh0, gw0, D, out.data_ptr(), gh, gw, _s(pos)))
    return out


def rope2d_table(grid, head_dim: int, theta: float = 100.0, device=None):
    """DINOv3's axial 2-D RoPE tables of a (gh, gw) patch grid (vdr_op_rope2d_table): (cos, sin), fp32 [gh*gw, head_dim/2]
    on the device."""
    lib = L.load()
    gh, gw = int(grid[0]), int(grid[1])
    dev = torch.device("cuda") if device is None else device
    cos = torch.empty((gh * gw, head_dim // 2), dtype=torch.float32, device=dev)
    sin = torch.empty_like(cos)
    L.check(lib.vdr_op_rope2d_table(gh, gw, int(head_dim), float(theta), cos.data_ptr(), sin.data_ptr(), _s(cos)))
    return cos, sin


def rope2d(qkv: torch.Tensor, batch: int, seq: int, prefix: int, heads: int, head_dim: int, cos: torch.Tensor,
           sin: torch.Tensor) -> torch.Tensor:
    """In place (vdr_op_rope2d): q and k of rows b*seq + prefix + j of the packed qkv [batch*seq, 3*heads*head_dim] bf16
    rotated with table row j; prefix rows and v untouched.  Returns qkv."""
    lib = L.load()
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    assert tuple(qkv.shape) == (batch * seq, 3 * heads * head_dim)
    for t in (cos, sin):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (seq - prefix, head_dim // 2)
    L.check(lib.vdr_op_rope2d(qkv.data_ptr(), batch, seq, prefix, heads, head_dim, cos.data_ptr(), sin.data_ptr(), _s(qkv)))
    return qkv


def interpolate_rel_pos(table: torch.Tensor, L_out: int) -> torch.Tensor:
    """table [L0, D] fp32 on the device -> [L_out, D] fp32: segment_anything's get_rel_pos resampling
    (vdr_op_interpolate_rel_pos: linear, align_corners=False, fp64 arithmetic, one rounding)."""
    lib = L.load()
    assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
    L0, D = table.shape
    out = torch.empty((int(L_out), D), dtype=torch.float32, device=table.device)
    L.check(lib.vdr_op_interpolate_rel_pos(table.data_ptr(), L0, D, out.data_ptr(), int(L_out), _s(table)))
    return out


def attention_relpos(qkv: torch.Tensor, rel_pos_h: torch.Tensor, rel_pos_w: torch.Tensor, batch: int, S: int, heads: int):
    """SAM attention with decomposed relative position bias over `batch` windows/grids of S x S tokens, 1 <= S <= 64."""
    if not 1 <= int(S) <= 64:
        raise ValueError(f"attention_relpos: S must be in 1..64, got {S}")
    lib = L.load()
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    assert qkv.shape == (batch * S * S, 3 * heads * 64)
    assert rel_pos_h.shape == (2 * S - 1, 64) and rel_pos_w.shape == (2 * S - 1, 64)
    npad = 2 * ((2 * S - 1 + 31) // 32 * 32)
    rel = torch.empty(batch * S * S * heads * npad + npad * 32, dtype=torch.float32, device=qkv.device)
    out = torch.empty((batch * S * S, heads * 64), dtype=torch.bfloat16, device=qkv.device)
    L.check(lib.vdr_op_attention_relpos(qkv.data_ptr(), rel_pos_h.float().contiguous().data_ptr(),
                                        rel_pos_w.float().contiguous().data_ptr(), rel.data_ptr(), out.data_ptr(), batch, S,
                                        heads, _s(qkv)))
    return out


def window_rows(batch: int, g: int, ws: int) -> int:
    """Rows of the window-partition order of `batch` g x g grids in ws x ws windows (border windows padded)."""
    nw = -(-g // ws)
    return batch * nw * nw * ws * ws


def layernorm_window(x: torch.Tensor, gamma, beta, eps: float, batch: int, g: int, ws: int, out=None) -> torch.Tensor:
    """norm1 + window_partition of a SAM block (vdr_op_layernorm_window): x bf16 [batch*g*g, D] in token order -> bf16
    [window_rows, D] in segment_anything's window_partition order.  Padding rows are not written: `out` (default: zeros)
    keeps what it held there."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[0] == batch * g * g
    D = x.shape[1]
    if out is None:
        out = torch.zeros((window_rows(batch, g, ws), D), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (window_rows(batch, g, ws), D)
    L.check(lib.vdr_op_layernorm_window(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), batch, g, ws, D,
                                        float(eps), _s(x)))
    return out


def layernorm_mx_window(x: torch.Tensor, gamma, beta, eps: float, batch: int, g: int, ws: int, out: MxTensor = None) -> MxTensor:
    """The same with MX-fp8 output (vdr_op_layernorm_mx_window): an MxTensor of window_rows rows; padding rows of the
    payload and the scales are not written (default `out`: zeroed, as the forward zeroes them)."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[0] == batch * g * g
    D = x.shape[1]
    rows = window_rows(batch, g, ws)
    if out is None:
        out = MxTensor.empty(rows, D, x.device)
        out.q.zero_()
    assert tuple(out.q.shape) == (rows, D) and out.scales.numel() == int(lib.vdr_mx_scale_bytes(rows, D))
    L.check(lib.vdr_op_layernorm_mx_window(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), batch, g, ws, D,
                                           out.q.data_ptr(), out.scales.data_ptr(), _s(x)))
    return out


def linear_window(x: torch.Tensor, W: torch.Tensor, bias, resid: torch.Tensor, batch: int, g: int, ws: int, variant=0,
                  out=None, part=None) -> torch.Tensor:
    """attn.proj + window_unpartition + residual of a SAM block (vdr_op_linear_window): x bf16 [window_rows, K] in
    windowed order, W bf16 [N, K], bias fp32 [N] or None, resid bf16 [batch*g*g, N] in token order -> out (default: a new
    tensor; may be resid) = resid + unpartition(x W^T + bias).  part fp32 [N/64, stride, 2]: the LayerNorm partials of
    out's rows, by token-order row."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and W.dtype == torch.bfloat16 and W.is_contiguous()
    N, K = W.shape
    assert tuple(x.shape) == (window_rows(batch, g, ws), K)
    assert resid.dtype == torch.bfloat16 and resid.is_contiguous() and tuple(resid.shape) == (batch * g * g, N)
    if out is None:
        out = torch.empty_like(resid)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (batch * g * g, N)
    L.check(lib.vdr_op_linear_window(x.data_ptr(), W.data_ptr(), _p(bias), resid.data_ptr(), out.data_ptr(), batch, g, ws, N, K,
                                     variant, _p(part), 0 if part is None else part.shape[1], _s(x)))
    return out


def im2col3(x: torch.Tensor, batch: int, g: int, out=None) -> torch.Tensor:
    """The SAM neck's 3 x 3 / padding 1 im2col (vdr_op_im2col3): x bf16 [batch*g*g, C] NHWC tokens -> bf16
    [batch*g*g, 9*C], tap-major (column (ky*3 + kx)*C + c)."""
    lib = L.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[0] == batch * g * g
    C_ = x.shape[1]
    if out is None:
        out = torch.empty((batch * g * g, 9 * C_), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (batch * g * g, 9 * C_)
    L.check(lib.vdr_op_im2col3(x.data_ptr(), out.data_ptr(), batch, g, C_, _s(x)))
    return out
