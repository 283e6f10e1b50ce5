"""The float64 softmax, the derived fp32 error bounds and the block-input read-back of the attention-map tests (TEST
HELPER): tests/test_attn_maps_gpu.py derives and uses them, tests/test_clip_model_gpu.py applies them to the CLIP /
SigLIP towers."""
import math

import torch

LOG2E = 1.4426950408889634


def softmax64(q, k, dh):
    return torch.softmax(q.double() @ k.double().transpose(-1, -2) / math.sqrt(dh), dim=-1)


def fp32_bounds(q, k, dh, N):
    """Entry-wise relative and |sum p - 1| bounds of the fp32 arithmetic against float64 of the same bf16 values.
    u = 2^-24.  The products q_i k_i of bf16 values are exact in fp32; their fp32 sum errs by at most
    (dh - 1) u sum_i |q_i k_i| <= dh u A (A = max over rows and keys of sum |q_i k_i|).  c = RN(RN(dh^-1/2) RN(log2 e)) is
    within 3u of dh^-1/2 log2 e, t = RN(s c) adds u |t|: |dt| <= c dh u A + 4 u T (T = max |t|); the same for m, and
    t - m adds u 2T: the exponent errs by at most E = 2 (c dh u A + 4 u T) + 2 u T.  v_exp_f32 is within 2 ulp (2^-22
    relative), so e is within ln2 E + 2^-22 relative.  l sums N such terms in fp32: N u more; r = RN(1/l) and p = RN(e r)
    add 2u.  So |p / p64 - 1| <= 2 (ln2 E + 2^-22) + (N + 2) u (the e error enters through e and l), and the row sum,
    N roundings of p more, |sum p - 1| <= that + N u.  Doubled for margin."""
    u = 2.0 ** -24
    c = LOG2E / math.sqrt(dh)
    A = float((q.abs() @ k.abs().transpose(-1, -2)).max())
    T = A * c
    E = 2 * (c * dh * u * A + 4 * u * T) + 2 * u * T
    rel = 2 * (math.log(2) * E + 2.0 ** -22) + (N + 2) * u
    return 2 * rel, 2 * (rel + N * u)


def block_input(e, x, layer):
    """the raw residual stream block `layer` reads, fp32 [B, N, D], from the library's own output"""
    import vdr
    return e.forward_layers(x, [vdr.LayerOut(layer - 1, vdr.OUT_TOKENS, torch.float32, norm=False)])[0]
