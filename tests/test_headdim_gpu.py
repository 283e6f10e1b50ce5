"""GPU: attention at head dims 32, 96 and 128 (csrc/attention_hd.hip) -- the op against an fp32 reference over sequence
lengths and batch sizes, its independence of the batch and of the padding, head dim 64 through the new entry point,
and the models that use it: the Stage-C classifiers on golden vectors made by the reference's own classes
(tests/golden/make_golden_headdim.py), variable-length batches, and a small pre-LN ViT."""
import io
import math
import os

import numpy as np
import pytest
import torch

import handle_configs as hc
from fixtures import ops  # noqa: F401
from model_gates import check_parity, gate_l2, min_cos, rel_l2
from ops_checks import BF16_EPS, assert_close, assert_unbiased, bf
from oracle import attn_designs as ad
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

HEAD_DIMS = (32, 96, 128)


def _ref(qkv, B, N, H, dh):
    """softmax(q k^T / sqrt(dh)) v in float64 on the device, [B*N, H*dh] (float64 on the host)"""
    q, k, v = qkv.cuda().double().reshape(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B * N, H * dh).cpu()


# ---- the op ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", HEAD_DIMS)
@pytest.mark.parametrize("N", [1, 5, 31, 32, 33, 127, 128, 129, 197, 288, 289, 577, 1024])
def test_attention_hd_sequence_lengths(ops, dh, N):
    B, H = 2, 3
    g = torch.Generator().manual_seed(dh * 10000 + N)
    qkv = bf(torch.randn(B * N, 3 * H * dh, generator=g))
    o = ops.attention(qkv.cuda(), B, N, H, head_dim=dh)
    ref = _ref(qkv, B, N, H, dh)
    # P is rounded to bf16 before P.V and the output is stored as bf16: 2^-8 relative on O(1) values
    assert_close(o, ref, 2 * BF16_EPS, 6e-3, f"attention dh{dh} B{B} N{N} H{H}")
    assert_unbiased(o, ref, f"attention dh{dh} B{B} N{N} H{H}")


@pytest.mark.parametrize("dh", HEAD_DIMS)
@pytest.mark.parametrize("B,N,H", [(1, 197, 1), (3, 197, 4), (130, 197, 4), (260, 300, 2), (1030, 50, 1)])
def test_attention_hd_batch_heads(ops, dh, B, N, H):
    """from one (sequence, head) item to more than 512"""
    g = torch.Generator().manual_seed(dh + B * 7 + N)
    qkv = bf(torch.randn(B * N, 3 * H * dh, generator=g))
    o = ops.attention(qkv.cuda(), B, N, H, head_dim=dh)
    ref = _ref(qkv, B, N, H, dh)
    assert_close(o, ref, 2 * BF16_EPS, 6e-3, f"attention dh{dh} B{B} N{N} H{H}")
    assert_unbiased(o, ref, f"attention dh{dh} B{B} N{N} H{H}")


@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_hd_rescale_branch_is_exercised(ops, dh):
    """The running max jumps at a late key chunk: one key far along the sequence matches query 7 strongly."""
    B, N, H = 1, 400, 1
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * N, 3 * dh, generator=g) * 0.3
    q = qkv[:, :dh]
    qkv[390, dh:2 * dh] = 4.0 * torch.sign(q[7])
    qkv[7, :dh] = 3.0 * torch.sign(q[7])
    qkv = bf(qkv)
    ref = _ref(qkv, B, N, H, dh)
    assert ref[7].abs().max() > 0  # (sanity)
    o = ops.attention(qkv.cuda(), B, N, H, head_dim=dh)
    assert_close(o, ref, 2 * BF16_EPS, 6e-3, f"attention rescale dh{dh}")


@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_hd_rows_sum_to_one(ops, dh):
    """V = all ones: every output is 1 whatever the scores."""
    B, N, H = 4, 197, 3
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B * N, 3 * H * dh, generator=g) * 2.0
    qkv[:, 2 * H * dh:] = 1.0
    o = ops.attention(bf(qkv).cuda(), B, N, H, head_dim=dh)
    assert_close(o, torch.ones(B * N, H * dh), 0.0, 4e-3, f"rows sum to one dh{dh}")


@pytest.mark.parametrize("dh", HEAD_DIMS)
@pytest.mark.parametrize("N", [33, 197, 577])
def test_attention_hd_sequence_output_does_not_depend_on_the_batch(ops, dh, N):
    H = 2
    B = 300  # 600 items
    g = torch.Generator().manual_seed(dh + N)
    qkv = bf(torch.randn(B * N, 3 * H * dh, generator=g)).cuda()
    full = ops.attention(qkv, B, N, H, head_dim=dh)
    for b in (0, 1, 157, B - 1):
        alone = ops.attention(qkv[b * N:(b + 1) * N].contiguous(), 1, N, H, head_dim=dh)
        assert torch.equal(alone, full[b * N:(b + 1) * N]), (dh, N, b)
    sub = ops.attention(qkv[:3 * N].contiguous(), 3, N, H, head_dim=dh)
    assert torch.equal(sub, full[:3 * N])
    for v in (1, 2, 3, 4):  # every variant is the same kernel
        assert torch.equal(ops.attention(qkv[:3 * N].contiguous(), 3, N, H, variant=v, head_dim=dh), sub)


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (43, 197, 12), (1, 577, 2), (3, 50, 4)])
def test_attention_hd_at_head_dim_64_is_vdr_op_attention(ops, B, N, H):
    import vdr
    from vdr.ops import _s
    lib = vdr.load()
    g = torch.Generator().manual_seed(B + N)
    qkv = bf(torch.randn(B * N, 3 * H * 64, generator=g)).cuda()
    for variant in (0, 1, 3):
        a = torch.empty((B * N, H * 64), dtype=torch.bfloat16, device="cuda")
        b = torch.full_like(a, 5.0)
        assert lib.vdr_op_attention(qkv.data_ptr(), a.data_ptr(), B, N, H, variant, _s(qkv)) == 0
        assert lib.vdr_op_attention_hd(qkv.data_ptr(), b.data_ptr(), B, N, H, 64, variant, _s(qkv)) == 0
        assert torch.equal(a, b), (B, N, H, variant)
    assert lib.vdr_op_attention_hd(qkv.data_ptr(), a.data_ptr(), B, N, H, 80, 0, _s(qkv)) == -7
    with pytest.raises(vdr.VdrError):
        ops.attention(qkv[:, : 3 * H * 48].contiguous(), B, N, H, head_dim=48)


# ---- models ---------------------------------------------------------------------------------------------
def _reference_state_dict(w, layers):
    sd = {"cls_token": w["cls_token"], "norm.weight": w["input_norm.weight"], "norm.bias": w["input_norm.bias"]}
    for i in range(layers):
        s, d = f"blocks.{i}.", f"transformer_encoder.layers.{i}."
        sd[d + "self_attn.in_proj_weight"] = w[s + "attn.qkv.weight"]
        sd[d + "self_attn.in_proj_bias"] = w[s + "attn.qkv.bias"]
        sd[d + "self_attn.out_proj.weight"] = w[s + "attn.proj.weight"]
        sd[d + "self_attn.out_proj.bias"] = w[s + "attn.proj.bias"]
        sd[d + "linear1.weight"], sd[d + "linear1.bias"] = w[s + "mlp.fc1.weight"], w[s + "mlp.fc1.bias"]
        sd[d + "linear2.weight"], sd[d + "linear2.bias"] = w[s + "mlp.fc2.weight"], w[s + "mlp.fc2.bias"]
        for n in ("norm1", "norm2"):
            sd[d + n + ".weight"], sd[d + n + ".bias"] = w[s + n + ".weight"], w[s + n + ".bias"]
    return sd


@pytest.mark.parametrize("tag", ["hd96", "hd32", "hd128"])
def test_golden_reference_classifier_at_head_dim(golden_dir, tag):
    """models_archs.TransformerNoduleClassifier golden vectors at dh = 96 / 32 / 128: the drop-in constructed with the
    reference signature, then load_state_dict in the reference's key names."""
    import vdr
    g = np.load(os.path.join(golden_dir, f"postln_{tag}.npz"), allow_pickle=False)
    dim, heads, layers, ffn = int(g["dim"]), int(g["heads"]), int(g["layers"]), int(g["ffn"])
    cfg = vo.postln_cfg(dim, heads, layers, ffn)
    w = vo.make_weights(cfg, seed=int(g["wseed"]), scale=float(g["wscale"]))
    x = vo.make_tokens(int(g["batch"]), int(g["seq"]), dim, seed=int(g["xseed"]))
    emu = vo.forward_tokens(cfg, w, x, emulate_bf16=True)
    sd = _reference_state_dict(w, layers)
    for k in ("dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias"):
        sd["classifier." + k] = torch.from_numpy(g["head.classifier." + k])
    m = vdr.TransformerNoduleClassifier(input_dim=dim, dim_feedforward=ffn, num_heads=heads, num_classes=2, num_layers=layers)
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    m.load_state_dict(torch.load(buf, map_location="cuda", weights_only=True))
    logits, cls = m(x.cuda())
    check_parity(cls, torch.from_numpy(g["cls"]), f"golden postln_{tag} cls", gate_l2(layers), emu["cls"])
    err = (logits.cpu() - torch.from_numpy(g["logits"])).abs().max().item()
    assert err < 3e-2, f"logits max abs err {err}"


def test_golden_reference_bimodal_classifier_at_head_dims(golden_dir):
    """TransformerNoduleBimodalClassifier at D 384: CT engine dh 96, PET engine dh 128, both cross attentions dh 96."""
    import vdr
    from oracle import bimodal_oracle as bo
    g = np.load(os.path.join(golden_dir, "bimodal_hd.npz"), allow_pickle=False)
    dim, lc, lp = int(g["dim"]), int(g["layers_ct"]), int(g["layers_pet"])
    rc, rp, hc, hp, ncls = float(g["ratio_ct"]), float(g["ratio_pet"]), int(g["heads_ct"]), int(g["heads_pet"]), int(g["classes"])
    sd = bo.make_state_dict(dim, int(rc * dim), int(rp * dim), lc, lp, ncls, seed=int(g["seed"]))
    m = vdr.TransformerNoduleBimodalClassifier(dim, rc, rp, hc, hp, lc, lp, ncls)
    m.load_state_dict(sd)
    x_ct, x_pet = torch.from_numpy(g["x_ct"]).cuda(), torch.from_numpy(g["x_pet"]).cuda()
    L = max(lc, lp) + 1
    for mode, (a, b) in (("both", (x_ct, x_pet)), ("ct", (x_ct, None)), ("pet", (None, x_pet))):
        out = m(a, b)
        for name, o in zip(("logits_petct", "cls_petct", "logits_ct", "logits_pet"), out):
            want = torch.from_numpy(g[f"{mode}_{name}"])
            assert o.shape == want.shape, (mode, name)
            if name.startswith("cls"):
                r, c = rel_l2(o.cpu(), want), min_cos(o.cpu(), want)
                print(f"bimodal_hd {mode} {name}: relL2 {r:.3e} min cos {c:.6f}")
                assert r <= gate_l2(L) and c >= 0.999, (mode, name, r, c)
            else:
                # 3e-2 absolute as for the other fixtures, scaled by the logits' size: at D 384 the seeded heads give
                # logits up to 3.4 (0.3-1.4 in bimodal_refdim), and bf16 rounding of the weights and inputs alone moves
                # them by 0.7 % rel L2 in fp32 arithmetic -- 0.012 absolute here against 0.003 there
                err = (o.cpu() - want).abs().max().item()
                assert err < 3e-2 * max(1.0, want.abs().max().item()), (mode, name, err)


def test_variable_length_sequences_at_head_dim_96():
    """Padded to the longest and run in one call (per-sequence key masking): every CLS row matches the oracle for that
    sequence alone and the GPU's one-at-a-time result, and does not depend on the padding contents, bit for bit."""
    import vdr
    dim, heads, layers, ffn = 384, 4, 2, 1536
    lens = [1, 37, 300, 129, 513, 64]
    cfg = vo.postln_cfg(dim, heads, layers, ffn)
    w = vo.make_weights(cfg, seed=13, scale=0.05)
    e = hc.engine(cfg, w)
    S = max(lens)
    seqs = [vo.make_tokens(1, n, dim, seed=200 + i)[0] for i, n in enumerate(lens)]
    pad = torch.full((len(lens), S, dim), 3.0)
    for i, t in enumerate(seqs):
        pad[i, : t.shape[0]] = t
    got = e.forward_tokens(pad.cuda(), vdr.OUT_CLS, lengths=lens).float().cpu()
    for i, t in enumerate(seqs):
        ref = vo.forward_tokens(cfg, w, t[None])["cls"][0]
        one = e.forward_tokens(t[None].cuda(), vdr.OUT_CLS).float().cpu()[0]
        r_ref, r_one = rel_l2(got[i][None], ref[None]), rel_l2(got[i][None], one[None])
        assert r_ref <= gate_l2(layers) and r_one <= 4e-3, (i, lens[i], r_ref, r_one)
    pad2 = pad.clone()
    for i, t in enumerate(seqs):
        pad2[i, t.shape[0]:] = -7.5
    assert torch.equal(got, e.forward_tokens(pad2.cuda(), vdr.OUT_CLS, lengths=lens).float().cpu())
    # the drop-in class takes the lengths the same way
    sd = _reference_state_dict(w, layers)
    gen = torch.Generator().manual_seed(3)
    sd.update({"classifier.dense1.weight": torch.randn(2 * dim, dim, generator=gen) * 0.05,
               "classifier.dense1.bias": torch.zeros(2 * dim),
               "classifier.dense2.weight": torch.randn(2, 2 * dim, generator=gen) * 0.05, "classifier.dense2.bias": torch.zeros(2)})
    m = vdr.TransformerNoduleClassifier(dim, ffn, heads, 2, layers, state_dict=sd)
    assert torch.equal(m(pad2.cuda(), lengths=lens)[1], e.forward_tokens(pad.cuda(), vdr.OUT_CLS, torch.float32, lengths=lens))


def test_small_preln_vit_at_head_dim_96():
    """bf16 pre-LN image model, D 192 / 2 heads (dh 96), CLS and dense tokens against the oracle."""
    import vdr
    cfg = vo.VitCfg(64, 16, 3, 192, 2, 2, 768)
    w = vo.make_weights(cfg, seed=3, scale=0.05)
    x = vo.make_images(cfg, 5, seed=4)
    ref = vo.forward_images(cfg, w, x)
    emu = vo.forward_images(cfg, w, x, emulate_bf16=True)
    e = hc.engine(cfg, w)
    g = gate_l2(cfg.layers)
    check_parity(e.forward(x.cuda(), vdr.OUT_CLS), ref["cls"], "vit dh96 cls", g, emu["cls"])
    check_parity(e.forward(x.cuda(), vdr.OUT_DENSE), ref["dense"], "vit dh96 dense", g, emu["dense"])
