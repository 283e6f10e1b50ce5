"""Checks and small references that the operator tests share (TEST HELPER): bf16 rounding, the elementwise tolerance
check, the bias check of oracle/attn_designs.py, "the same fp32 bits", and the float64 SAM rel-pos attention."""
import torch

from oracle import attn_designs as ad

BF16_EPS = 2.0 ** -8


def bf(x):
    return x.to(torch.bfloat16)


def assert_close(got, ref, rtol, atol, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = err > bound
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside tol; first at {i}: got "
                             f"{got[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g}; max err {err.max().item():.4g}")


def assert_unbiased(got, ref, what):
    """beta = <got - ref, ref> / <ref, ref> against the float64 reference, |beta| <= 3e-4 from 30 k outputs on
    (oracle/attn_designs.py): rounding noise gives ~1e-5; a softmax temperature, P rounding or denominator error moves
    every output the same way and gives 1e-3 and more, inside the elementwise tolerance"""
    b = ad.check_unbiased(got.detach().double().cpu(), ref, what)
    if b is not None:
        print(f"beta {what}: {b:+.3e}")


def assert_same_bits(a, b, what, dtype=torch.float32):
    """a and b are tensors of `dtype` (32 bits wide) and one shape with the same bits everywhere; reports the count, the
    first positions and the values that differ"""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == dtype and b.dtype == dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    same = a.view(torch.int32) == b.view(torch.int32)
    assert bool(same.all()), (what, int((~same).sum()), torch.nonzero(~same)[:4].tolist(),
                              a[~same][:4].tolist(), b[~same][:4].tolist())


def relpos_attn_ref(qkv, rel_h, rel_w, B, S, H):
    """float64"""
    from oracle import sam_oracle as so
    q, k, v = qkv.double().reshape(B, S * S, 3, H, 64).permute(2, 0, 3, 1, 4)
    attn = (q * 0.125) @ k.transpose(-1, -2)
    Rh, Rw = so.rel_table(S, rel_h.double()), so.rel_table(S, rel_w.double())
    rq = q.reshape(B, H, S, S, 64)
    rh = torch.einsum("bnhwc,hkc->bnhwk", rq, Rh)
    rw = torch.einsum("bnhwc,wkc->bnhwk", rq, Rw)
    attn = (attn.view(B, H, S, S, S, S) + rh[..., :, None] + rw[..., None, :]).view(B, H, S * S, S * S)
    o = torch.softmax(attn, dim=-1) @ v
    return o.transpose(1, 2).reshape(B * S * S, H * 64)
