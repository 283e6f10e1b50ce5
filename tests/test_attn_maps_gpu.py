"""GPU: attention maps -- vdr_op_attention_probs at op level on designed inputs with exactly known outputs, and
vdr_forward_attn_maps / VitDescriptorModel inside the forward.

The kernel's arithmetic (include/vdr.h): s = q.k in fp32, t = s * c, m = max t, e = exp2(t - m), l = sum e, p = e * RN(1/l);
head_mean: (sum of p over the heads in head order) * RN(1/H).  So Q = 0 gives exactly RN(1/seq) everywhere, and a query
that is a large multiple of one key (every other exp2 underflows) gives exactly 1.0 there and 0 elsewhere."""
import math

import pytest
import torch

import handle_configs as hc
from attn_maps_ref import LOG2E, block_input, fp32_bounds, softmax64
from fixtures import ops  # noqa: F401
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

DHS = (32, 64, 96, 128)
SEQS = (1, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197, 257, 577, 1025)


def _qkv(B, N, H, dh, q, k, v):
    """packed [B*N, 3*H*dh] bf16 from q, k, v [B, H, N, dh]"""
    t = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4)  # B, N, 3, H, dh
    return t.reshape(B * N, 3 * H * dh).to(torch.bfloat16).cuda().contiguous()


def _signs(gen, shape):
    return torch.randint(0, 2, shape, generator=gen).float() * 2 - 1


def _distinct_sign_keys(gen, B, H, N, dh):
    k = _signs(gen, (B, H, N, dh))
    while True:  # every key row distinct: another key's dot with the chosen one is at most dh - 2
        flat = k.reshape(B * H, N, dh)
        dup = False
        for r in flat:
            if torch.unique(r, dim=0).shape[0] != N:
                dup = True
        if not dup:
            return k
        k = _signs(gen, (B, H, N, dh))


def _q_rows_set(N):
    return sorted({1, min(7, N), N})


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("N", SEQS)
def test_uniform_rows_are_exactly_one_over_seq(ops, dh, N):
    """Q = 0: every score is 0, e = 1, l = N, p = RN(1/N) -- in every row, head, layout and dtype."""
    gen = torch.Generator().manual_seed(N * 7 + dh)
    B, H = 2, 2
    q = torch.zeros(B, H, N, dh)
    k, v = torch.randn(B, H, N, dh, generator=gen), torch.randn(B, H, N, dh, generator=gen)
    qkv = _qkv(B, N, H, dh, q, k, v)
    r = torch.tensor(1.0, dtype=torch.float32) / N
    for qr in _q_rows_set(N):
        for mean in (False, True):
            got = ops.attention_probs(qkv, B, N, H, dh, qr, mean, torch.float32).cpu()
            assert got.shape == ((B, qr, N) if mean else (B, H, qr, N))
            assert torch.all(got == r), (qr, mean, got.unique()[:5])
            gb = ops.attention_probs(qkv, B, N, H, dh, qr, mean, torch.bfloat16).cpu()
            assert gb.dtype == torch.bfloat16 and torch.all(gb == r.to(torch.bfloat16)), (qr, mean)


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("N", SEQS)
def test_one_hot_rows_pin_key_order_rows_and_heads(ops, dh, N):
    """Q_i = 1024 K_pi(i) with distinct +-1 keys: s = 1024 dh at pi(i), at most 1024 (dh - 2) elsewhere -- a gap of
    2048 c >= 261 in log2 units, so every other exp2 underflows to 0: entry pi(i) is exactly 1.0, all others exactly 0.
    pi differs per (sequence, head): a wrong key order, query row, head or chunk boundary moves a 1."""
    gen = torch.Generator().manual_seed(1000 + N * 7 + dh)
    B, H = 2, 4
    k = _distinct_sign_keys(gen, B, H, N, dh)
    pi = torch.randint(0, N, (B, H, N), generator=gen)
    q = 1024.0 * torch.gather(k, 2, pi[..., None].expand(B, H, N, dh))
    qkv = _qkv(B, N, H, dh, q, k, torch.randn(B, H, N, dh, generator=gen))
    want = torch.nn.functional.one_hot(pi, N).float()  # [B, H, N, N]
    for qr in _q_rows_set(N):
        got = ops.attention_probs(qkv, B, N, H, dh, qr, False, torch.float32).cpu()
        assert torch.equal(got, want[:, :, :qr]), qr
        gb = ops.attention_probs(qkv, B, N, H, dh, qr, False, torch.bfloat16).cpu()
        assert torch.equal(gb.float(), want[:, :, :qr]), qr
        # H = 4, a power of two: the mean of one-hot heads is exact
        mean = ops.attention_probs(qkv, B, N, H, dh, qr, True, torch.float32).cpu()
        assert torch.equal(mean, want[:, :, :qr].sum(1) * 0.25), qr


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("N", (2, 33, 197, 577))
def test_two_way_tie_is_exactly_one_half(ops, dh, N):
    """Two identical keys that both win: e = 1 at both, l = 2, p = 0.5 exactly."""
    gen = torch.Generator().manual_seed(77 + N + dh)
    B, H = 1, 2
    k = _distinct_sign_keys(gen, B, H, N, dh)
    a, b = 0, N - 1
    k[:, :, b] = k[:, :, a]
    q = 1024.0 * k[:, :, a:a + 1].expand(B, H, N, dh)
    qkv = _qkv(B, N, H, dh, q, k, torch.randn(B, H, N, dh, generator=gen))
    got = ops.attention_probs(qkv, B, N, H, dh, N, False, torch.float32).cpu()
    want = torch.zeros(B, H, N, N)
    want[..., a] = 0.5
    want[..., b] = 0.5
    assert torch.equal(got, want)


def _random_qkv(gen, B, N, H, dh, amp):
    """bf16 q, k uniform in [-amp, amp] (|s| <= dh amp^2), v ~ N(0, 1)"""
    q = ((torch.rand(B, H, N, dh, generator=gen) * 2 - 1) * amp).to(torch.bfloat16).float()
    k = ((torch.rand(B, H, N, dh, generator=gen) * 2 - 1) * amp).to(torch.bfloat16).float()
    v = torch.randn(B, H, N, dh, generator=gen).to(torch.bfloat16).float()
    return q, k, v


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("N", (5, 65, 197, 577, 1025))
def test_random_rows_against_a_float64_softmax(ops, dh, N):
    gen = torch.Generator().manual_seed(5 * N + dh)
    B, H = 2, 3
    q, k, v = _random_qkv(gen, B, N, H, dh, amp=2.0)
    qkv = _qkv(B, N, H, dh, q, k, v)
    ref = softmax64(q, k, dh)
    rel_b, sum_b = fp32_bounds(q, k, dh, N)
    got = ops.attention_probs(qkv, B, N, H, dh, N, False, torch.float32).cpu().double()
    rel = ((got - ref).abs() / ref).max().item()
    assert rel <= rel_b, (rel, rel_b)
    assert (got.sum(-1) - 1).abs().max().item() <= sum_b
    assert ref.max() > 1.5 / N  # (the rows are not uniform: the check has something to see)
    # head_mean, bitwise against the rule applied to the per-head output: (p_0 + p_1 + p_2) * RN(1/3) in fp32
    qr = min(7, N)
    ph = ops.attention_probs(qkv, B, N, H, dh, qr, False, torch.float32)
    acc = ph[:, 0].clone()
    for h in range(1, H):
        acc = acc + ph[:, h]
    want = acc * (torch.tensor(1.0, dtype=torch.float32, device=acc.device) / H)
    assert torch.equal(ops.attention_probs(qkv, B, N, H, dh, qr, True, torch.float32), want)
    # bf16 output is one RNE rounding of the fp32 value
    assert torch.equal(ops.attention_probs(qkv, B, N, H, dh, qr, True, torch.bfloat16), want.to(torch.bfloat16))
    assert torch.equal(ops.attention_probs(qkv, B, N, H, dh, qr, False, torch.bfloat16), ph.to(torch.bfloat16))


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("N", (33, 197, 577))
def test_map_times_v_matches_the_fused_attention(ops, dh, N):
    """P V in float64 from the map and the bf16 V matches vdr_op_attention* on the same qkv within the fused kernel's bf16
    rounding of P (2^-9 relative per entry) and of its output (2^-9 relative)."""
    gen = torch.Generator().manual_seed(11 * N + dh)
    B, H = 2, 2
    q, k, v = _random_qkv(gen, B, N, H, dh, amp=1.0)
    qkv = _qkv(B, N, H, dh, q, k, v)
    p = ops.attention_probs(qkv, B, N, H, dh, N, False, torch.float32).cpu().double()
    pv = p @ v.double()  # [B, H, N, dh]
    fused = ops.attention(qkv, B, N, H, head_dim=dh).cpu().double().reshape(B, N, H, dh).permute(0, 2, 1, 3)
    tol = 2.0 ** -8 * (p @ v.double().abs()) + 2.0 ** -8 * pv.abs() + 1e-6
    assert torch.all((fused - pv).abs() <= tol), ((fused - pv).abs() / tol).max()


@pytest.mark.parametrize("dh", DHS)
def test_invariance_batch_repeat_and_cls_row(ops, dh):
    """A sequence's map is bitwise the same alone or inside a larger batch and in repeated launches; the q_rows = 1 map is
    bitwise row 0 of the full map."""
    gen = torch.Generator().manual_seed(dh)
    B, N, H = 5, 197, 3
    q, k, v = _random_qkv(gen, B, N, H, dh, amp=1.0)
    qkv = _qkv(B, N, H, dh, q, k, v)
    for mean in (False, True):
        full = ops.attention_probs(qkv, B, N, H, dh, N, mean)
        assert torch.equal(full, ops.attention_probs(qkv, B, N, H, dh, N, mean))
        alone = ops.attention_probs(qkv[3 * N:4 * N].contiguous(), 1, N, H, dh, N, mean)
        assert torch.equal(alone[0], full[3])
        cls = ops.attention_probs(qkv, B, N, H, dh, 1, mean)
        assert torch.equal(cls, full[:, :1] if mean else full[:, :, :1])


# ---- inside the forward --------------------------------------------------------------------------------------------

VIT3 = vo.VitCfg(64, 16, 3, 128, 2, 3, 512)  # dh 64, N = 17
PATHS = {"fold": dict(), "no_ln_fold": dict(ln_fold=False), "fp8": dict(fp8=1), "resid_fp32": dict(resid_fp32=True),
         "fp8_cls_bf16": dict(fp8=1, fp8_cls_bf16=True)}


def _peaked(cfg, seed, gain):
    """seeded weights whose q / k rows are scaled by `gain`: attention far from uniform"""
    w = vo.make_weights(cfg, seed=seed, scale=0.05)
    D = cfg.dim
    for i in range(cfg.layers):
        w[f"blocks.{i}.attn.qkv.weight"][:2 * D] *= gain
    return w


@pytest.mark.parametrize("path", sorted(PATHS))
def test_zeroed_heads_are_exactly_uniform_inside_the_forward(path):
    """q rows and bias of head 1 of block 1 set to zero: that head's map is exactly RN(1/N) for any image, whatever the
    path; head 0 is not uniform."""
    import vdr
    cfg = VIT3
    w = _peaked(cfg, 5, 4.0)
    dh = cfg.dim // cfg.heads
    w["blocks.1.attn.qkv.weight"][dh:2 * dh] = 0
    w["blocks.1.attn.qkv.bias"][dh:2 * dh] = 0
    e = hc.engine(cfg, w, **PATHS[path])
    N = cfg.n_tokens
    x = vo.make_images(cfg, 3, seed=2).cuda()
    _, (full, cls) = e.forward_attn_maps(x, [vdr.AttnMap(1, N), vdr.AttnMap(1, 1, dtype=torch.bfloat16)])
    r = torch.tensor(1.0 / N, dtype=torch.float32)
    assert torch.all(full[:, 1].cpu() == r)
    assert torch.all(cls[:, 1].cpu() == r.to(torch.bfloat16))
    assert (full[:, 0] - r.cuda()).abs().max() > 0.05


@pytest.mark.parametrize("dh", (32, 64, 96, 128))
def test_maps_match_a_recompute_on_the_explicit_layernorm_path(ops, dh):
    """no_ln_fold: block l's input from the library's raw stream, norm1 by the library's LayerNorm op (the forward's kernel:
    the same bf16 rows), then qkv = h W^T + b and the softmax in float64.  The forward stores q / k as bf16 roundings of an
    fp32 GEMM that errs by at most K u sum_j |h_j W_j| (+ u |b|): where that interval holds no bf16 rounding boundary
    the stored value IS the rounding of the float64 value; elsewhere it may be its neighbour (one ulp).  The score bound
    is the sum of those possible flips, |ds| <= sum over ambiguous i of ulp(q_i) |k_i| + |q_i| ulp(k_i) + ulp ulp, plus the
    fp32 softmax bound of the op tests: |p_k - p64_k| <= p64_k (2^(c (ds_k + max_j ds_j)) - 1) + the fp32 term.  Summed over a map's entries,
    two heads' (and two layers') maps are at least 10x that bound apart, so the comparison tells them apart."""
    import vdr
    D = dh * 2
    cfg = vo.VitCfg(64, 16, 3, D, 2, 3, 2 * D)
    w = _peaked(cfg, 7 + dh, math.sqrt(1200.0 / D))  # scores of about 3 nats spread at every width
    e = hc.engine(cfg, w, ln_fold=False)
    N, H = cfg.n_tokens, cfg.heads
    x = vo.make_images(cfg, 3, seed=9).cuda()
    c = LOG2E / math.sqrt(dh)
    maps = {}
    bounds = {}
    for layer in (1, 2):
        _, (got,) = e.forward_attn_maps(x, [vdr.AttnMap(layer, N)])
        xin = block_input(e, x, layer).reshape(-1, D).to(torch.bfloat16).contiguous()
        h = ops.layernorm(xin, w[f"blocks.{layer}.norm1.weight"].cuda(), w[f"blocks.{layer}.norm1.bias"].cuda(), cfg.ln_eps,
                          torch.bfloat16).double()
        W = w[f"blocks.{layer}.attn.qkv.weight"].to(torch.bfloat16).double().cuda()
        bias = w[f"blocks.{layer}.attn.qkv.bias"].double().cuda()
        y = h @ W.T + bias
        err = (D + 2) * 2.0 ** -24 * (h.abs() @ W.abs().T + bias.abs())
        rn = y.to(torch.bfloat16)
        lo, hi = (y - err).to(torch.bfloat16), (y + err).to(torch.bfloat16)
        amb = (lo != rn) | (hi != rn)  # the stored value may be rn's neighbour
        mag = rn.double().abs().clamp_min(2.0 ** -126)
        ulp = torch.where(amb, torch.exp2(torch.floor(torch.log2(mag)) - 7), torch.zeros_like(y))  # bf16 spacing at rn
        B = x.shape[0]
        qk = rn.double().reshape(B, N, 3, H, dh)
        uq = ulp.reshape(B, N, 3, H, dh)
        q, k = qk[:, :, 0].transpose(1, 2), qk[:, :, 1].transpose(1, 2)
        dq, dk = uq[:, :, 0].transpose(1, 2), uq[:, :, 1].transpose(1, 2)
        ds = dq @ k.abs().transpose(-1, -2) + q.abs() @ dk.transpose(-1, -2) + dq @ dk.transpose(-1, -2)
        ref = softmax64(q, k, dh)
        rel_b, _ = fp32_bounds(q.cpu(), k.cpu(), dh, N)
        # log2 p_k = t_k - log2 sum_j 2^t_j moves by at most c (ds_k + max_j ds_j)
        dmax = ds.max(-1, keepdim=True).values
        bound = ref * (torch.exp2(c * (ds + dmax)) - 1) + ref * rel_b + 1e-7
        got64 = got.double()
        assert torch.all((got64 - ref).abs() <= bound), ((got64 - ref).abs() / bound).max()
        ent = -(ref * ref.clamp_min(1e-300).log()).sum(-1).mean().item()
        assert ent < 0.8 * math.log(N), ent  # far from uniform
        maps[layer], bounds[layer] = got64, bound
    # summed over the entries of a map: the distance to another head's (another layer's) map against 10x the bound
    for layer in (1, 2):
        b = bounds[layer]
        assert (maps[layer][:, 0] - maps[layer][:, 1]).abs().sum() >= 10 * (b[:, 0] + b[:, 1]).sum()
    assert (maps[1] - maps[2]).abs().sum() >= 10 * (bounds[1] + bounds[2]).sum()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_features_are_bitwise_those_of_forward_layers(path):
    import vdr
    cfg = VIT3
    w = _peaked(cfg, 3, 2.0)
    e = hc.engine(cfg, w, **PATHS[path])
    x = vo.make_images(cfg, 4, seed=1).cuda()
    specs = [vdr.LayerOut(0, vdr.OUT_TOKENS, norm=False), vdr.LayerOut(1, vdr.OUT_DENSE, torch.bfloat16),
             vdr.LayerOut(2, vdr.OUT_CLS), vdr.LayerOut(2, vdr.OUT_POOLED)]
    want = e.forward_layers(x, specs)
    feats, maps = e.forward_attn_maps(x, [vdr.AttnMap(0, 1), vdr.AttnMap(2, cfg.n_tokens, True)], specs)
    for a, b in zip(feats, want):
        assert torch.equal(a, b)
    assert maps[0].shape == (4, cfg.heads, 1, cfg.n_tokens) and maps[1].shape == (4, cfg.n_tokens, cfg.n_tokens)


def test_maps_do_not_depend_on_how_the_batch_is_run():
    """micro_batch / streams, batch size and duplicate images: bitwise the same maps."""
    import vdr
    cfg = VIT3
    w = _peaked(cfg, 4, 4.0)
    N = cfg.n_tokens
    x = vo.make_images(cfg, 7, seed=3).cuda()
    req = [vdr.AttnMap(0, N), vdr.AttnMap(1, 1, True), vdr.AttnMap(2, 5, False, torch.bfloat16)]
    ref = hc.engine(cfg, w).forward_attn_maps(x, req)[1]
    for kw in (dict(micro_batch=3), dict(micro_batch=2, streams=3), dict(micro_batch=1, streams=2)):
        got = hc.engine(cfg, w, **kw).forward_attn_maps(x, req)[1]
        for a, b in zip(got, ref):
            assert torch.equal(a, b), kw
    e = hc.engine(cfg, w)
    sub = e.forward_attn_maps(x[2:5].contiguous(), req)[1]
    for a, b in zip(sub, ref):
        assert torch.equal(a, b[2:5])
    dup = e.forward_attn_maps(torch.stack([x[4], x[4], x[4]]), req)[1]
    for a, b in zip(dup, ref):
        for i in range(3):
            assert torch.equal(a[i], b[4])


@pytest.mark.parametrize("path", ["fold", "no_ln_fold", "fp8", "fp8_cls_bf16"])
def test_last_block_map_with_cls_only_outputs(path):
    """A map of the last block beside CLS outputs of that block: the block runs its CLS rows only after the attention
    (block_tail_cls).  The map equals the map of a call whose last block runs every row, the CLS features equal
    forward_layers', and a map-only last block stops after its attention with the same map."""
    import vdr
    cfg = VIT3
    w = _peaked(cfg, 6, 4.0)
    e = hc.engine(cfg, w, **PATHS[path])
    N, L = cfg.n_tokens, cfg.layers
    x = vo.make_images(cfg, 3, seed=5).cuda()
    req = [vdr.AttnMap(L - 1, N), vdr.AttnMap(L - 1, 1, True)]
    feats, maps = e.forward_attn_maps(x, req, [vdr.LayerOut(L - 1, vdr.OUT_CLS)])
    _, maps_full = e.forward_attn_maps(x, req, [vdr.LayerOut(L - 1, vdr.OUT_TOKENS)])
    _, maps_only = e.forward_attn_maps(x, req)
    for a, b, c in zip(maps, maps_full, maps_only):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(feats[0], e.forward_layers(x, [vdr.LayerOut(L - 1, vdr.OUT_CLS)])[0])
    assert torch.equal(feats[0], e.forward(x, vdr.OUT_CLS))
    # the head-mean CLS row is the mean of the per-head CLS rows (the rule, in fp32)
    acc = maps[0][:, 0, :1].clone()
    for h in range(1, cfg.heads):
        acc = acc + maps[0][:, h, :1]
    assert torch.equal(maps[1], acc * (torch.tensor(1.0, dtype=torch.float32, device=acc.device) / cfg.heads))


def test_model_level_checks_of_layer_and_q_rows():
    import vdr
    cfg = VIT3
    e = hc.engine(cfg, _peaked(cfg, 1, 1.0))
    x = vo.make_images(cfg, 1, seed=0).cuda()
    lib = vdr.load()
    for bad in (vdr.AttnMap(3), vdr.AttnMap(-1)):
        with pytest.raises(vdr.VdrError, match="layer"):
            e.forward_attn_maps(x, [bad], [])
        assert b"maps[0]" in lib.vdr_last_error(e.h)
    with pytest.raises(ValueError, match="q_rows"):
        e.forward_attn_maps(x, [vdr.AttnMap(0, cfg.n_tokens + 1)])


def test_python_methods_shapes_and_layouts():
    import vdr
    cfg = VIT3
    w = _peaked(cfg, 8, 4.0)
    m = vdr.VitDescriptorModel(hc.vit_config(cfg), w)
    B, H, N, g = 2, cfg.heads, cfg.n_tokens, cfg.img // cfg.patch
    x = vo.make_images(cfg, B, seed=6).cuda()
    last = m.get_last_selfattention(x)
    assert last.shape == (B, H, N, N) and last.dtype == torch.float32
    assert torch.allclose(last.sum(-1), torch.ones(B, H, N, device=last.device), atol=1e-5)
    cls = m.get_attention_maps(x)
    assert cls.shape == (B, H, N) and torch.equal(cls, last[:, :, 0])
    heat = m.get_attention_maps(x, reshape=True)
    assert heat.shape == (B, H, g, g) and torch.equal(heat, last[:, :, 0, 1:].reshape(B, H, g, g))
    hm = m.get_attention_maps(x, head_mean=True, reshape=True)
    assert hm.shape == (B, g, g)
    l0, l2 = m.get_attention_maps(x, layers=[0, 2], cls_only=False, head_mean=True)
    assert l0.shape == (B, N, N) and l2.shape == (B, N, N)
    assert torch.equal(m.get_attention_maps(x, layers=2, cls_only=False), last)
    assert m.get_attention_maps(x, layers=[2, 0], cls_only=False, head_mean=True)[1].shape == (B, N, N)
