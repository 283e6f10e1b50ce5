"""The model-level parity gate and the batch-property check (TEST HELPER): the one statement of both, used by every
test that compares a forward against an oracle.  tests/test_model_gates_cpu.py shows on the CPU that each assertion
rejects what it is meant to reject.

Stated tolerances (SURVEY.md 8d "Parity gate"; derivation in tests/test_model_gpu.py's docstring), for L layers:
per-row cosine >= 0.999 and relative L2 <= gate_l2(L) = 4e-3 + 3e-3 sqrt(max(L, 1)), against the fp32 oracle and
against the restatement that emulates bf16 rounding at the device's store points."""
import math

import torch


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def min_cos(a, b):
    a, b = a.double().reshape(-1, a.shape[-1]), b.double().reshape(-1, b.shape[-1])
    return torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()


def gate_l2(layers):
    return 4e-3 + 3e-3 * math.sqrt(max(layers, 1))


def gate_l2_fp8(layers):
    return 4e-2 + 4e-2 * math.sqrt(max(layers, 1))


def check_parity(got, ref, what, l2, ref_emul=None, l2_emul=None, cos=0.999, emul="bf16-emulating"):
    """got (any device / dtype) against ref, and against ref_emul when given (gate l2_emul, default l2).  Nothing is
    reshaped: (a - b).norm() broadcasts, so a caller whose output has another layout reshapes it itself."""
    got = got.float().cpu()
    l2_emul = l2 if l2_emul is None else l2_emul
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: not finite"
    r, c = rel_l2(got, ref), min_cos(got, ref)
    re = None if ref_emul is None else rel_l2(got, ref_emul)
    print(f"{what}: relL2 vs fp32 {r:.3e} (gate {l2:.3e})" + ("" if re is None else f"  vs {emul} {re:.3e} (gate {l2_emul:.3e})")
          + f"  min row cosine {c:.6f} (gate {cos})")
    assert c >= cos, f"{what}: min cosine {c} < {cos}"
    assert r <= l2, f"{what}: rel L2 vs fp32 reference {r} > {l2}"
    if re is not None:
        assert re <= l2_emul, f"{what}: rel L2 vs {emul} reference {re} > {l2_emul}"


def check_parity_fp8(got, ref, ref_mx, layers, what):
    """fp8 gates: cosine >= 0.99 per row against the fp32 oracle (the reference has no fp8 path, so
    this is parity with its fp32 arithmetic) and relative L2 <= 4e-2 + 4e-2 sqrt(L): an e4m3 element carries
    ~2.5 % rms rounding error, a K-long dot product of two such operands ~3.5 %, diluted by the residual
    stream, four quantised linears per block (measured 6.9e-2 .. 7.9e-2 at L = 2 .. 3).  The oracle that emulates the same MX-fp8 quantisation points is printed
    and gated at the same level, not tighter: the quantiser itself is bit-exact (tests/test_ops_gpu.py), but any
    bf16-level difference upstream moves elements across e4m3 rounding boundaries (6 % each), so two correct
    runs decorrelate to roughly the quantisation noise itself."""
    check_parity(got, ref, what, gate_l2_fp8(layers), ref_emul=ref_mx, cos=0.99, emul="MX-emulating")


def check_batch_properties(run, x, small=3, perm=None, lo=None):
    """run(x) -> tensor, x [B, ...] on its device with x[B-1] == x[1]: the output is finite, duplicate images give bitwise
    equal rows, a batch permutation (seeded by B unless given) permutes the rows, and rows lo : lo + small (lo = B // 2
    unless given) do not depend on the batch they travel in.  Returns run(x)."""
    B = x.shape[0]
    out = run(x)
    assert torch.isfinite(out.float()).all(), "not finite"
    assert torch.equal(out[B - 1], out[1]), "duplicate images must give bitwise equal rows"
    if perm is None:
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    perm = torch.as_tensor(perm).to(x.device)
    assert torch.equal(run(x[perm].contiguous()), out[perm]), "batch permutation equivariance"
    lo = B // 2 if lo is None else lo
    assert torch.equal(run(x[lo:lo + small].contiguous()), out[lo:lo + small]), "a row depends on its batch"
    return out


def inject_outlier_channels(w, layers, dim, seed, fc1_key):
    """What trained DINOv2-g / SAM checkpoints carry and seeded Gaussian weights do not ("massive activations"): a few
    LayerNorm gains of 30-100x, and residual-stream channels that sit at 10^2..10^3 in every token.  The columns of the
    linears that read those channels are scaled down by the same factors, as a trained model's are -- otherwise q.k^T
    saturates every softmax and ANY bf16 implementation decorrelates from fp32 arithmetic by argmax flips, which would
    test nothing of this library.  What is left is what the checkpoints stress here: row variances formed as
    E[x^2] - mean^2 from fp32 partial sums with one term 10^4..10^5 x the others, bf16 rounding of rows whose mean is far
    from 0, and MX blocks of 32 whose shared e8m0 scale is set by one outlier."""
    g = torch.Generator().manual_seed(seed)
    ch = torch.randperm(dim, generator=g)[:5].tolist()
    gains = {ch[0]: 30.0, ch[1]: 60.0, ch[2]: 100.0}
    w = {k: v.clone() for k, v in w.items()}
    w["patch_embed.proj.bias"][ch[3]] += 300.0   # every token carries +300 / -120 in these channels into every block
    w["patch_embed.proj.bias"][ch[4]] -= 120.0
    for i in range(layers):
        for norm, lin in (("norm1", "attn.qkv"), ("norm2", fc1_key)):
            for c, gain in gains.items():
                w[f"blocks.{i}.{norm}.weight"][c] *= gain
                w[f"blocks.{i}.{lin}.weight"][:, c] /= gain
            # the normalised value of a +300 channel is ~ 300 / sqrt(300^2 / D) = sqrt(D): keep its products ordinary
            w[f"blocks.{i}.{lin}.weight"][:, ch[3]] /= math.sqrt(dim)
            w[f"blocks.{i}.{lin}.weight"][:, ch[4]] /= math.sqrt(dim) * 0.4
    return w, ch
