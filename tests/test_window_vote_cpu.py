"""CPU: the multi-source soft window vote without a device -- vdr_op_window_vote is declared, bound and exported and refuses
bad arguments, naming the op, before it touches a device, and vdr.ops.window_vote mirrors every refusal as ValueError;
vdr.local.vote_window, the torch statement of the op, against the float64 restatement and DINO's dense form
(tests/window_vote_ref.py) inside the bound derived there, against vdr.local.topk + vdr.knn.vote for one source and hard
labels, and on planted ties; the host-side refusals of VitDescriptorModel.propagate_volume."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import local_corr_ref as lref
import window_vote_ref as wref

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(os.path.dirname(HERE), "include", "vdr.h")
INF = float("inf")

# (P, S, grid, r, k, C): one source and several, k at the corner maximum, one class, the widest row
CASES = ((2, 1, (5, 7), 2, 5, 3), (1, 3, (4, 4), 1, 12, 2), (2, 8, (3, 5), 4, 16, 5), (1, 2, (6, 6), 2, 9, 1), (1, 8, (9, 17), 8, 16, 8))


def test_header_binding_and_exports_declare_the_window_vote():
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"int vdr_op_window_vote\(const float\* cost, const float\* src, int problems, int sources, int gh, int gw, "
                     r"int radius, int k,\s*int n_classes, int weights, float temperature, float\* scores, int32_t\* labels, "
                     r"int32_t\* idx, float\* val,\s*void\* stream\);", src)
    for name, value in (("VDR_WINDOW_VOTE_MAX_SOURCES", 8), ("VDR_WINDOW_VOTE_MAX_K", 16), ("VDR_WINDOW_VOTE_MAX_CLASSES", 64),
                        ("VDR_VOTE_SOFTMAX", 0), ("VDR_VOTE_UNIFORM", 1), ("VDR_ABI_VERSION", 8)):
        assert re.search(rf"#define {name} {value}\b", src), name
    assert "vdr_op_window_vote" in _lib.SYMBOLS and hasattr(_lib.load(), "vdr_op_window_vote")
    import vdr
    from vdr import ops
    assert (ops.WINDOW_VOTE_MAX_SOURCES, ops.WINDOW_VOTE_MAX_K, ops.WINDOW_VOTE_MAX_CLASSES) == (8, 16, 64)
    assert ops.VOTE_WEIGHTS == ("softmax", "uniform") and callable(ops.window_vote) and callable(vdr.local.vote_window)
    assert callable(vdr.VitDescriptorModel.propagate_volume)
    assert [f for f in vdr.VolumePropagation.__dataclass_fields__][:5] == ["scores", "labels", "grid", "radius", "index"]


def test_op_window_vote_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    cost, src, scores, labels, idx, val = (base + 1024 * n for n in range(6))

    def call(cost=cost, src=src, P=2, S=2, gh=2, gw=3, r=1, k=3, Cn=4, w=0, T=0.1, scores=scores, labels=labels, idx=idx, val=val):
        return lib.vdr_op_window_vote(cost, src, P, S, gh, gw, r, k, Cn, w, T, scores, labels, idx, val, None)

    def refused(code, kw, word=None):
        assert call(**kw) == code, kw
        msg = lib.vdr_last_error(None)
        assert msg.startswith(b"window_vote: "), (kw, msg)
        assert word is None or word in msg, (kw, msg)

    for kw in (dict(cost=None), dict(src=None), dict(scores=None)):
        refused(-1, kw, b"null pointer")
    for kw in (dict(P=0), dict(P=-1), dict(S=0), dict(S=-2), dict(gh=0), dict(gw=0), dict(gh=-3), dict(Cn=0), dict(Cn=-4)):
        refused(-1, kw, b"positive")
    for kw in (dict(cost=cost + 4), dict(src=src + 8), dict(scores=scores + 12)):
        refused(-1, kw, b"16-byte aligned")
    for kw in (dict(labels=labels + 4), dict(idx=idx + 8), dict(val=val + 4)):
        refused(-1, kw, b"labels, idx and val must be 16-byte aligned")
    refused(-1, dict(P=2 ** 12, S=8, gh=2 ** 8, gw=2 ** 8), b"problems * sources * gh * gw exceeds")
    for kw in (dict(gh=2 ** 16, gw=2 ** 16, P=1, S=1), dict(gh=2 ** 20, gw=2 ** 20, P=1, S=1)):
        refused(-1, kw, b"exceeds 2^31 - 1")
    for S in (9, 64):
        refused(-7, dict(S=S), b"sources must be 1 .. 8")  # VDR_ERR_UNSUPPORTED
    for r in (0, -1, 9, 100):
        refused(-7, dict(r=r), b"radius must be 1 .. 8")
    for k in (0, -1, 17, 100):
        refused(-7, dict(k=k), b"k must be 1 .. 16")
    for Cn in (65, 1000):
        refused(-7, dict(Cn=Cn), b"n_classes must be 1 .. 64")
    # the in-grid candidates of a corner patch: S * min(gh, r + 1) * min(gw, r + 1)
    for kw, n in ((dict(k=9), 8), (dict(S=1, k=5), 4), (dict(S=1, gh=1, gw=1, k=2, r=8), 1), (dict(S=1, gh=5, gw=7, r=2, k=10), 9)):
        refused(-1, kw, b"k exceeds the %d in-grid candidates" % n)
    for w in (2, -1):
        refused(-1, dict(w=w), b"weights must be VDR_VOTE_SOFTMAX or VDR_VOTE_UNIFORM")
    for T in (0.0, -0.1, INF, -INF, float("nan")):
        refused(-1, dict(T=T), b"temperature must be positive and finite")
        refused(-1, dict(T=T, w=1), b"temperature")
    for kw in (dict(idx=None), dict(val=None)):
        refused(-1, kw, b"idx and val must both be given or both be null")
    refused(-1, dict(P=1, S=8, gh=2 ** 10, gw=2 ** 10, r=8, k=1), b"(2 radius + 1)^2 exceeds")
    refused(-1, dict(P=8, S=8, gh=2 ** 10, gw=2 ** 9, r=1, k=1, Cn=64), b"n_classes exceeds")
    # the order: null before sizes, sizes before ranges, ranges before the corner rule, that before weights, temperature, outputs
    refused(-1, dict(cost=None, gh=0, S=9), b"null pointer")
    refused(-1, dict(gh=0, S=9, k=0), b"positive")
    refused(-7, dict(S=9, r=0, k=0, Cn=65), b"sources")
    refused(-7, dict(r=0, k=0, Cn=65), b"radius")
    refused(-7, dict(k=0, Cn=65), b"k must be")
    refused(-7, dict(Cn=65, k=9), b"n_classes")
    refused(-1, dict(k=9, w=2, T=0.0), b"k exceeds")
    refused(-1, dict(w=2, T=0.0, idx=None), b"weights")
    refused(-1, dict(T=0.0, idx=None), b"temperature")
    # (the well-formed variants -- null labels, null idx and val together, uniform weights -- run in tests/test_window_vote_gpu.py)


def test_ops_window_vote_mirrors_every_refusal_as_value_error():
    from vdr import local, ops
    cost, src = wref.random_inputs(2, 2, (2, 3), 1, 4, seed=1)
    for fn, name in ((ops.window_vote, "window_vote"), (local.vote_window, "vote_window")):
        def bad(match, c=cost, s=src, grid=(2, 3), k=3, **kw):
            with pytest.raises(ValueError, match=match) as e:
                fn(c, s, grid, k, **kw)
            assert str(e.value).startswith(name + ": "), e.value

        bad("cost must be", c=cost[0])
        bad("cost must be", c=cost.double())
        bad("cost must be", c=None)
        bad("src must be", s=src[0])
        bad("src must be", s=src.long())
        bad("agree in P, S and t", s=src[:1])
        bad("agree in P, S and t", s=src[:, :1])
        bad("must be positive", c=cost[:0], s=src[:0])
        bad("must be positive", s=src[..., :0])
        bad("must be positive", grid=(0, 3))
        bad("rows, the grid", grid=(3, 3))
        bad("sources must be 1 .. 8", c=cost[:, :1].expand(2, 9, 6, 9), s=src[:, :1].expand(2, 9, 6, 4))
        bad(r"for no radius in 1\.\.8", c=cost[..., :8])
        bad(r"for no radius in 1\.\.8", c=torch.zeros(2, 2, 6, 19 * 19))
        for k in (0, -1, 17, 1.5, True):
            bad("k must be an integer in 1 .. 16", k=k)
        bad("n_classes must be 1 .. 64", s=src[..., :1].expand(2, 2, 6, 65))
        bad("k exceeds the 8 in-grid candidates", k=9)
        bad("k exceeds the 4 in-grid candidates", c=cost[:, :1], s=src[:, :1], k=5)
        bad("weights must be one of", weights="softmx")
        for T in (0.0, -1.0, INF, float("nan"), 1e-60):  # (1e-60 is 0 in fp32, the type the op takes)
            bad("temperature must be positive and finite", temperature=T)
    with pytest.raises(ValueError, match="on the device"):
        ops.window_vote(cost, src, (2, 3), 3)  # CPU tensors: vote_window is what runs there


def _torch_vote(cost, src, grid, k, **kw):
    from vdr import local
    scores, labels, idx, val = local.vote_window(cost, src, grid, k, **kw)
    assert scores.dtype == torch.float32 and labels.dtype == torch.int32 and idx.dtype == torch.int32 and val.dtype == torch.float32
    P, S, t, C = src.shape
    assert tuple(scores.shape) == (P, t, C) and tuple(labels.shape) == (P, t) and tuple(idx.shape) == tuple(val.shape) == (P, t, k)
    return scores.numpy(), labels.numpy(), idx.numpy(), val.numpy()


@pytest.mark.parametrize("weights,T", (("softmax", 0.1), ("softmax", 0.01), ("uniform", 0.1)))
@pytest.mark.parametrize("P,S,grid,r,k,C", CASES)
def test_vote_window_equals_the_restatement_inside_the_bound(P, S, grid, r, k, C, weights, T):
    cost, src = wref.random_inputs(P, S, grid, r, C, seed=7 + S)
    scores, labels, idx, val = _torch_vote(cost, src, grid, k, weights=weights, temperature=T)
    want, want_lab, want_idx, want_val = wref.vote(cost, src, grid, k, weights, T)
    bnd = wref.bound(cost, src, grid, k, weights, T)
    assert np.array_equal(idx, want_idx) and np.array_equal(val.astype(np.float64), want_val)
    ratio = np.abs(scores - want) / bnd
    clear = wref.margin_clear(want, bnd)
    print(f"S {S} grid {grid} r {r} k {k} C {C} {weights} T {T}: worst error / bound {ratio.max():.3f}, clear rows {clear.mean():.3f}")
    assert (ratio <= 1.0).all()
    assert np.array_equal(labels[clear], want_lab[clear])
    # every neighbour is inside its patch's window, in its own source
    t = grid[0] * grid[1]
    for m in range(k):
        lref.slot_of(idx[..., m].astype(np.int64) % t, grid, r)
    assert (idx >= 0).all() and (idx < S * t).all()


@pytest.mark.parametrize("P,S,grid,r,k,C", CASES)
def test_vote_window_equals_dinos_dense_form_where_the_kth_value_is_not_tied(P, S, grid, r, k, C):
    cost, src = wref.random_inputs(P, S, grid, r, C, seed=11 + S)
    want, no_tie = wref.dino_dense(cost, src, grid, k, 0.1)
    print(f"S {S} grid {grid} r {r} k {k}: share of rows without a tie at the k-th value {no_tie.mean():.4f}")
    assert no_tie.mean() >= 0.95  # at most 5 % of the rows may be excluded
    scores = _torch_vote(cost, src, grid, k, temperature=0.1)[0]
    bnd = wref.bound(cost, src, grid, k, "softmax", 0.1)
    assert (np.abs(scores - want)[no_tie] <= bnd[no_tie]).all()
    # and the two float64 forms are one number there
    assert np.abs(wref.vote(cost, src, grid, k, "softmax", 0.1)[0] - want)[no_tie].max() < 1e-12


@pytest.mark.parametrize("grid,r,k,C", (((5, 7), 2, 5, 4), ((4, 4), 4, 16, 3), ((1, 6), 1, 1, 2), ((9, 17), 8, 9, 6)))
@pytest.mark.parametrize("weights", ("softmax", "uniform"))
def test_one_source_with_hard_labels_is_topk_and_knn_vote(grid, r, k, C, weights):
    from vdr import knn, local
    cost, _ = wref.random_inputs(2, 1, grid, r, C, seed=5)
    t = grid[0] * grid[1]
    hard = torch.randint(0, C, (2, t), generator=torch.Generator().manual_seed(6))
    src = torch.nn.functional.one_hot(hard, C).float().unsqueeze(1)
    scores, labels, idx, val = local.vote_window(cost, src, grid, k, weights=weights, temperature=0.1)
    want_idx, want_val = local.topk(cost[:, 0], grid, k)
    assert torch.equal(idx, want_idx) and torch.equal(val, want_val)
    other = knn.vote(want_idx, want_val, hard, C, weights=weights, temperature=0.1)
    want = wref.vote(cost, src, grid, k, weights, 0.1)[0]
    knn_bound = wref.knn_vote_bound(want_val, want, weights, 0.1)
    both = wref.bound(cost, src, grid, k, weights, 0.1) + knn_bound
    assert (np.abs(scores.numpy() - other.numpy()) <= both).all()
    assert (np.abs(other.numpy() - want) <= knn_bound).all()  # (the bound granted to knn.vote holds for it)
    clear = wref.margin_clear(want, both)
    assert np.array_equal(labels.numpy()[clear], knn.lowest_argmax(other).numpy()[clear])


def _planted(S, grid, r, C=3):
    """a low random background below every planted value, -inf outside the grid"""
    cost, src = wref.random_inputs(1, S, grid, r, C, seed=2)
    return torch.where(torch.isfinite(cost), cost * 0.25 - 1.0, cost), src


def test_the_tie_order_is_value_then_source_then_slot():
    from vdr import local
    grid, r, t, WW = (5, 5), 1, 25, 9
    i = 12  # the centre patch: all 9 slots are inside the grid; slot w is patch j = i + (w // 3 - 1) * 5 + (w % 3 - 1)
    def j(w):
        return i + (w // 3 - 1) * 5 + (w % 3 - 1)
    # the same value in two sources: the lower source first, whatever the slots
    cost, src = _planted(3, grid, r)
    cost[0, 2, i, 1] = cost[0, 0, i, 7] = 0.5
    cost[0, 1, i, 4] = 0.75
    _, _, idx, val = local.vote_window(cost, src, grid, 3)
    assert idx[0, i].tolist() == [1 * t + j(4), 0 * t + j(7), 2 * t + j(1)] and val[0, i].tolist() == [0.75, 0.5, 0.5]
    # the same value in two slots of one source: the lower slot first
    cost, src = _planted(2, grid, r)
    cost[0, 1, i, 8] = cost[0, 1, i, 2] = cost[0, 1, i, 5] = 0.5
    _, _, idx, val = local.vote_window(cost, src, grid, 3)
    assert idx[0, i].tolist() == [t + j(2), t + j(5), t + j(8)] and val[0, i].tolist() == [0.5, 0.5, 0.5]
    # a tie that straddles the k-th place: exactly k are taken, the first of the tied ones under the order
    cost, src = _planted(3, grid, r)
    cost[0, 0, i, 3] = 0.9
    for s, w in ((2, 0), (1, 6), (1, 2), (0, 8)):
        cost[0, s, i, w] = 0.5
    for k, want in ((2, [(0, 3), (0, 8)]), (3, [(0, 3), (0, 8), (1, 2)]), (4, [(0, 3), (0, 8), (1, 2), (1, 6)])):
        scores, _, idx, val = local.vote_window(cost, src, grid, k, weights="uniform")
        assert idx[0, i].tolist() == [s * t + j(w) for s, w in want]
        mean = torch.stack([src[0, s, j(w)] for s, w in want]).double().mean(0)
        assert torch.allclose(scores[0, i].double(), mean, rtol=0, atol=k * 2.0 ** -23)
    # a corner patch ignores what the slots outside the grid hold: a huge finite value there is never selected
    cost, src = _planted(1, grid, r)
    cost[0, 0, 0, :] = torch.where(torch.isfinite(cost[0, 0, 0, :]), cost[0, 0, 0, :], torch.tensor(9.0))
    _, _, idx, _ = local.vote_window(cost, src, grid, 4)
    assert sorted(idx[0, 0].tolist()) == [0, 1, 5, 6]


def test_designed_inputs_are_exact_in_the_torch_statement():
    """what tests/test_window_vote_gpu.py asks of the kernel bit for bit holds for vote_window on the CPU"""
    for S, grid, r, k, C, dyadic in ((1, (2, 3), 1, 4, 2, True), (2, (5, 7), 4, 5, 5, False), (8, (3, 4), 8, 16, 64, True)):
        cost, src = wref.designed(2, S, grid, r, C, seed=3, dyadic=dyadic)
        for weights, T in (("softmax", 0.01), ("uniform", 0.1)):
            scores, labels, idx, val = _torch_vote(cost, src, grid, k, weights=weights, temperature=T)
            want, want_lab, want_idx, want_val = wref.vote(cost, src, grid, k, weights, T)
            # (the labels from the ROUNDED scores: float64 keeps weights of 1e-87 that fp32 does not, which can split a tie)
            assert np.array_equal(scores, want.astype(np.float32)) and np.array_equal(labels, want.astype(np.float32).argmax(-1))
            assert np.array_equal(idx, want_idx) and np.array_equal(val.astype(np.float64), want_val)


def _stub_model(cfg, grid=(2, 2), size=(32, 32), stride=16):
    """a VitDescriptorModel without an engine behind it: what the refusals read, nothing a device is needed for"""
    from vdr import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg, m.model_name, m.dynamic_size, m.device = cfg, "stub", False, torch.device("cpu")
    m.engine = types.SimpleNamespace(grid=grid, input_size=size, patch_stride=stride)
    return m


def test_propagate_volume_refusals_need_no_device():
    import vdr
    m = _stub_model(vdr.ARCHS["vit_tiny16_224"])
    x, lab = torch.zeros(4, 3, 32, 32), torch.zeros(2, 2, dtype=torch.int64)
    soft = torch.full((2, 2, 3), 1 / 3)

    def bad(match, x=x, labels=lab, n_classes=3, **kw):
        kw = {**dict(radius=1, k=1), **kw}
        with pytest.raises(ValueError, match=match) as e:
            m.propagate_volume(x, labels, n_classes, **kw)
        return e

    bad(r"\[B, 3, H, W\]", x=x[0])
    bad("input size in force", x=torch.zeros(4, 3, 48, 48))
    for r in (0, 9, -2, 1.5):
        bad("radius", radius=r)
    for i in (4, -1, 1.5, True):
        bad(r"index must be an integer in 0\.\.3", index=i)
    for n in (8, -1, 2.5):
        bad(r"n_context must be an integer in 0\.\.7", n_context=n)
    for d in ("forward", "", None):
        bad("direction must be", direction=d)
    for b in (0, -1, 1.5):
        bad("max_batch", max_batch=b)
    for labels in (lab[:1], lab.reshape(4), torch.zeros(2, 2, 3, dtype=torch.int64), lab.bool(), lab.float(), soft[..., :2], soft[:1], None):
        bad("labels must be", labels=labels)
    for labels in (lab + 3, lab - 1):
        bad(r"0\.\.2", labels=labels)
    for labels in (soft - 1.0, soft * INF, soft * float("nan")):
        bad("finite and non-negative", labels=labels)
    for k in (5, 0, -1, 1.5):  # a corner of the 2 x 2 grid has 4 candidates at any radius, and the first step one source
        bad("k must be", radius=4, k=k)
    for n in (0, 65):
        bad("n_classes", n_classes=n)
    for T in (0.0, -1.0, INF):
        bad("temperature", temperature=T)
    bad("facet", facet="keys")
    bad("hierarchy", bin=True, hierarchy=4)
    bad("out of range", layer=12)
    m.cfg = vdr.ARCHS["medsam"]
    bad("SAM")
    # k is held to the first step, which has one source, and to the op's 16
    big = _stub_model(vdr.ARCHS["vit_tiny16_224"], grid=(6, 6), size=(96, 96))
    with pytest.raises(ValueError, match=r"k must be 1\.\.16"):
        big.propagate_volume(torch.zeros(2, 3, 96, 96), torch.zeros(6, 6, dtype=torch.int64), 2, radius=8, k=17)
    with pytest.raises(ValueError, match=r"k must be 1\.\.9"):
        big.propagate_volume(torch.zeros(2, 3, 96, 96), torch.zeros(6, 6, dtype=torch.int64), 2, radius=2, k=10, n_context=7)
