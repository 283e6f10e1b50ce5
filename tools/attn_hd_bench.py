#!/usr/bin/env python3
"""Attention at head dims 32 / 64 / 96 / 128 (csrc/attention.hip for 64, csrc/attention_hd.hip for the others): time per
launch with HIP events after warm-up, at equal sequence length and equal (sequence, head) item count, and the achieved
rate against the 2.5 PF dense-bf16 peak (4 seq^2 dh FLOP per item).  Then the whole TransformerNoduleClassifier forward
at D 384 / 4 heads (dh 96) on a padded variable-length batch against the reference-shaped torch.nn.TransformerEncoder
(fp32 eager, same GPU), the two alternated in one process.

    python tools/attn_hd_bench.py [--out results.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-deep-radiomics_amd"))
import torch  # noqa: E402

import vdr  # noqa: E402
from vdr import ops  # noqa: E402

PEAK = 2.5e15  # dense bf16 FLOP/s, MI355X


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3  # median, min (us)


def op_table(rounds):
    rows = []
    for items, seq in ((3072, 197), (256, 600)):
        qkvs = {}
        for dh in (32, 64, 96, 128):
            g = torch.Generator(device="cuda").manual_seed(dh)
            qkvs[dh] = torch.randn(items * seq, 3 * dh, generator=g, device="cuda").to(torch.bfloat16)
        res = {dh: [] for dh in qkvs}
        for _ in range(rounds):  # the head dims alternate round by round
            for dh, q in qkvs.items():
                res[dh].append(timeit(lambda: ops.attention(q, items, seq, 1, head_dim=dh)))
        for dh in qkvs:
            med = sorted(r[0] for r in res[dh])[len(res[dh]) // 2]
            flop = 4.0 * seq * seq * dh * items
            rows.append(dict(items=items, seq=seq, head_dim=dh, us=round(med, 2), tflops=round(flop / med / 1e6, 1),
                             frac_peak=round(flop / med / 1e-6 / PEAK, 4)))
            print(f"items {items:5d} seq {seq:4d} dh {dh:3d}: {med:9.2f} us  {flop / med / 1e6:7.1f} TF/s  "
                  f"{flop / med / 1e-6 / PEAK:.3f} of peak", flush=True)
    return rows


def classifier(rounds, batch=64, dim=384, heads=4, layers=2, ffn=1536):
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(300, 1001, (batch,), generator=g).tolist()
    S = max(lens)
    x = torch.randn(batch, S, dim, generator=g)
    for i, n in enumerate(lens):
        x[i, n:] = 0.0
    xd = x.cuda()
    # the reference-shaped model (models_archs.TransformerNoduleClassifier: CLS token, input LayerNorm, post-LN encoder
    # with GELU, MLP head on the CLS row), fp32 eager, padding masked as keys
    enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(dim, heads, ffn, dropout=0.0, activation="gelu",
                                                                       batch_first=True), layers, enable_nested_tensor=False)
    norm = torch.nn.LayerNorm(dim)
    head = torch.nn.Sequential(torch.nn.Linear(dim, 2 * dim), torch.nn.GELU(), torch.nn.Linear(2 * dim, 2))
    cls_tok = torch.nn.Parameter(torch.randn(1, 1, dim, generator=g) * 0.02)
    with torch.no_grad():
        for name, p in list(enc.named_parameters()) + [("norm.weight", norm.weight), ("norm.bias", norm.bias)] + \
                list(head.named_parameters()):
            ln_gain = "norm" in name and name.endswith("weight")
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if ln_gain else 0.05) + (1.0 if ln_gain else 0.0))
    enc, norm, head = enc.cuda().eval(), norm.cuda().eval(), head.cuda().eval()
    cls_d = cls_tok.detach().cuda()
    mask = torch.zeros(batch, S + 1, dtype=torch.bool)
    for i, n in enumerate(lens):
        mask[i, n + 1:] = True
    mask = mask.cuda()

    def torch_fwd():
        with torch.no_grad():
            h = norm(torch.cat([cls_d.expand(batch, 1, dim), xd], dim=1))
            c = enc(h, src_key_padding_mask=mask)[:, 0]
            return head(c), c

    sd = {"cls_token": cls_tok.detach().reshape(1, 1, dim), "norm.weight": norm.weight.detach().cpu(),
          "norm.bias": norm.bias.detach().cpu()}
    for k, v in enc.state_dict().items():
        sd["transformer_encoder." + k] = v.detach().cpu()
    sd.update({"classifier.dense1.weight": head[0].weight.detach().cpu(), "classifier.dense1.bias": head[0].bias.detach().cpu(),
               "classifier.dense2.weight": head[2].weight.detach().cpu(), "classifier.dense2.bias": head[2].bias.detach().cpu()})
    m = vdr.TransformerNoduleClassifier(dim, ffn, heads, 2, layers, state_dict=sd)

    def vdr_fwd():
        return m(xd, lengths=lens)

    ours, ref = [], []
    for _ in range(rounds):
        ours.append(timeit(vdr_fwd, iters=10)[0])
        ref.append(timeit(torch_fwd, iters=10)[0])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    c_ours, c_ref = vdr_fwd()[1].float(), torch_fwd()[1].float()
    rel = ((c_ours - c_ref).norm() / c_ref.norm()).item()
    out = dict(batch=batch, dim=dim, heads=heads, layers=layers, ffn=ffn, tokens=sum(lens), max_len=S,
               vdr_ms=round(med(ours) / 1e3, 3), torch_fp32_ms=round(med(ref) / 1e3, 3),
               speedup=round(med(ref) / med(ours), 2), cls_rel_l2=round(rel, 5))
    print(f"classifier D{dim}/{heads} heads, {batch} sequences of 300..1000 tokens (padded to {S}): "
          f"vdr {out['vdr_ms']} ms, torch fp32 {out['torch_fp32_ms']} ms, x{out['speedup']}, CLS rel L2 {rel:.2e}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = dict(ops=op_table(a.rounds), classifier=classifier(a.rounds), device=torch.cuda.get_device_name(0),
               source_id=vdr._lib.source_id())
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
