"""CPU: the windowed correlation without a device -- vdr_op_local_correlation / vdr_local_correlation_work_bytes are declared,
bound and exported and refuse bad arguments, naming the op, before they touch a device; the mapping of csrc/local_corr_map.h
covers every (query, slot) exactly once (tests/local_corr_map_cases.cpp, a host program); the float64 restatement
(tests/local_corr_ref.py) equals its own brute-force loop; vdr.local's offsets, topk and soft_displacement on designed costs,
and soft_displacement on random costs inside the bound derived in the restatement; the host-side refusals of
propagate_labels and find_correspondences(radius=)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import host_program
import local_corr_ref as lref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "include", "vdr.h")
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")
INF = float("inf")


def test_header_binding_and_exports_declare_the_local_correlation_entry_points():
    from vdr import _lib
    src = open(HDR).read()
    assert re.search(r"size_t vdr_local_correlation_work_bytes\(int pairs, int gh, int gw, int radius\);", src)
    assert re.search(r"int vdr_op_local_correlation\(const void\* x, int64_t ldx, int64_t x_stride, const void\* y, int64_t ldy, "
                     r"int64_t y_stride,\s*int pairs, int gh, int gw, int d, int radius, int transposed, void\* work,\s*"
                     r"float\* cost, float\* best_sim, int32_t\* best_idx, void\* stream\);", src)
    assert re.search(r"#define VDR_LOCAL_CORR_MAX_RADIUS 8\b", src) and re.search(r"#define VDR_ABI_VERSION 8\b", src)
    assert {"vdr_op_local_correlation", "vdr_local_correlation_work_bytes"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_local_correlation") and hasattr(lib, "vdr_local_correlation_work_bytes")
    import vdr
    from vdr import ops
    assert ops.LOCAL_CORR_MAX_RADIUS == 8 and callable(ops.local_correlation) and callable(vdr.VitDescriptorModel.propagate_labels)
    assert callable(vdr.local.offsets) and callable(vdr.local.topk) and callable(vdr.local.soft_displacement)
    fields = [f for f in vdr.Correspondences.__dataclass_fields__]
    assert fields[:8] == ["nn12", "sim12", "nn21", "sim21", "saliency1", "saliency2", "mask", "grid"]
    assert vdr.Correspondences.radius is None and vdr.Correspondences.cost12 is None  # (attributes every result has)
    assert [f for f in vdr.Propagation.__dataclass_fields__][:4] == ["scores", "labels", "idx", "val"]


def test_op_local_correlation_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    x, y, work, cost, bs, bi = (base + 1024 * k for k in range(6))

    def call(x=x, ldx=32, xs=192, y=y, ldy=32, ys=192, pairs=2, gh=2, gw=3, d=32, r=1, tr=0, work=work, cost=cost, bs=bs, bi=bi):
        return lib.vdr_op_local_correlation(x, ldx, xs, y, ldy, ys, pairs, gh, gw, d, r, tr, work, cost, bs, bi, None)

    def refused(code, kw, word=None):
        assert call(**kw) == code, kw
        msg = lib.vdr_last_error(None)
        assert msg.startswith(b"local_correlation: "), (kw, msg)
        assert word is None or word in msg, (kw, msg)

    for kw in (dict(d=16, ldx=16, ldy=16), dict(d=48, ldx=48, ldy=48), dict(d=8), dict(d=33, ldx=40, ldy=40)):
        refused(-7, kw, b"multiple of 32")  # VDR_ERR_UNSUPPORTED
    for r in (0, -1, 9, 100):
        refused(-7, dict(r=r), b"radius")
    invalid = [dict(x=None), dict(y=None), dict(work=None), dict(pairs=0), dict(pairs=-1), dict(gh=0), dict(gw=0), dict(gh=-3), dict(gw=-1),
               dict(d=0), dict(d=-32), dict(ldx=24), dict(ldy=31), dict(d=64), dict(xs=-96), dict(ys=-8),
               dict(x=x + 2), dict(x=x + 8), dict(y=y + 4), dict(work=work + 8), dict(cost=cost + 4), dict(bs=bs + 8), dict(bi=bi + 12),
               dict(ldx=36), dict(ldy=44), dict(xs=100), dict(ys=68),
               dict(pairs=2, gh=2 ** 15, gw=2 ** 15), dict(pairs=1, gh=2 ** 16, gw=2 ** 16), dict(pairs=1, gh=2 ** 20, gw=2 ** 20),
               dict(cost=None, bs=None, bi=None), dict(bs=None), dict(bi=None), dict(cost=None, bs=None), dict(cost=None, bi=None),
               dict(pairs=1, gh=2 ** 12, gw=2 ** 12, r=8), dict(pairs=2 ** 10, gh=2 ** 9, gw=2 ** 9, r=1)]
    for kw in invalid:
        refused(-1, kw)  # VDR_ERR_INVALID
    # the order: a null pointer before the sizes, the sizes before d % 32, the operand before the radius, the radius before the outputs
    refused(-1, dict(x=None, gh=0, d=8, r=0), b"null pointer")
    refused(-1, dict(gh=0, d=8, r=0), b"positive")
    refused(-7, dict(d=8, r=0), b"multiple of 32")
    refused(-7, dict(r=0, cost=None, bs=None, bi=None), b"radius")
    refused(-1, dict(cost=None, bs=None, bi=None), b"no output")
    refused(-1, dict(pairs=1, gh=2 ** 12, gw=2 ** 12, r=8), b"(2 radius + 1)^2")
    # a stride of 0, a null cost and a null best pair are well formed: such a call gets as far as the device check or the launch
    assert call(ys=0, cost=None) in (0, -2, -3) and call(bs=None, bi=None, tr=1) in (0, -2, -3)


def test_work_bytes_is_positive_granular_and_monotone():
    from vdr import _lib
    wb = _lib.load().vdr_local_correlation_work_bytes
    for pairs in (1, 2, 3, 8, 64):
        for gh in (1, 2, 7, 8, 9, 14, 27, 63):
            for gw in (1, 5, 15, 16, 17, 63):
                for r in (1, 2, 4, 7, 8):
                    w = wb(pairs, gh, gw, r)
                    assert w > 0 and w % 16 == 0
                    # at least the two maps' row norms and the cost rows
                    assert w >= 4 * pairs * gh * gw * (2 + (2 * r + 1) ** 2)
                    assert wb(pairs + 1, gh, gw, r) > w and wb(pairs, gh + 1, gw, r) > w and wb(pairs, gh, gw + 1, r) > w
                    assert r == 8 or wb(pairs, gh, gw, r + 1) > w
    assert wb(0, 5, 5, 1) == 0 and wb(1, 0, 5, 1) == 0 and wb(1, 5, -1, 1) == 0 and wb(1, 5, 5, 0) == 0 and wb(1, 5, 5, 9) == 0


def test_the_mapping_covers_every_query_slot_once(tmp_path):
    """tests/local_corr_map_cases.cpp, a host program with its own main, over the header the kernel includes"""
    lines = host_program.run("local_corr_map_cases", tmp_path).splitlines()
    assert len(lines) == 17 * 4 and all(line.startswith("ok ") for line in lines)
    assert any(line.startswith("ok 1x1 r=8 ") for line in lines) and any(line.startswith("ok 9x17 r=4 ") for line in lines)


@pytest.mark.parametrize("r", (1, 2, 8))
@pytest.mark.parametrize("grid", ((1, 1), (1, 5), (3, 3), (5, 7)))
def test_the_restatement_equals_the_brute_force_loop(grid, r):
    t, d = grid[0] * grid[1], 32
    gen = torch.Generator().manual_seed(100 * t + r)
    x = torch.randn(2, t, d, generator=gen).to(torch.bfloat16)
    y = torch.randn(2, t, d, generator=gen).to(torch.bfloat16)
    if t >= 3:  # a tie inside a window: the lowest candidate wins in both
        y[:, 1] = y[:, 0]
    c = lref.cost(x, y, grid, r)
    bs, bi, slot = lref.best(c, grid, r)
    wc, wbs, wbi = lref.brute(x, y, grid, r)
    assert c.shape == (2, t, (2 * r + 1) ** 2)
    assert np.array_equal(np.isneginf(c), np.isneginf(wc))
    # (the gather takes an einsum's dot product, the loop numpy's dot: the same float64 definition in two summation orders)
    fin = np.isfinite(wc)
    assert np.abs(c[fin] - wc[fin]).max() < 1e-13
    assert np.abs(bs - wbs).max() < 1e-13 and np.array_equal(bi, wbi)
    assert np.array_equal(lref.slot_of(bi.astype(np.int64), grid, r), slot)
    b = lref.bound(x, y, grid, r)
    assert np.array_equal(b == 0.0, ~fin) and (b[fin] > 0).all()


def test_offsets_exactly():
    from vdr import local
    assert local.offsets(1).dtype == torch.int64
    assert local.offsets(1).tolist() == [[-1, -1], [-1, 0], [-1, 1], [0, -1], [0, 0], [0, 1], [1, -1], [1, 0], [1, 1]]
    for r in (2, 4, 8):
        o = local.offsets(r)
        W = 2 * r + 1
        assert tuple(o.shape) == (W * W, 2) and np.array_equal(o.numpy(), lref.offsets(r))
        assert o[0].tolist() == [-r, -r] and o[W * W // 2].tolist() == [0, 0] and o[-1].tolist() == [r, r] and o[1].tolist() == [-r, 1 - r]
    for bad in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="radius"):
            local.offsets(bad)


def test_topk_on_designed_costs():
    from vdr import local
    grid, r = (2, 3), 1
    j, ok = lref.window(2, 3, 1)
    c = np.where(ok, 0.0, -INF)[None].astype(np.float32)  # every in-grid slot ties at 0
    c[0, 4, 4] = 0.5    # the centre patch (1, 1): itself, slot (0, 0) ...
    c[0, 4, 0] = 0.5    # ... ties with its neighbour at (-1, -1), the lower slot
    c[0, 4, 5] = 0.75   # and (0, +1) beats both
    idx, val = local.topk(torch.from_numpy(c), grid, 4)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == (1, 6, 4)
    assert idx[0, 4].tolist() == [5, 0, 4, 1] and val[0, 4].tolist() == [0.75, 0.5, 0.5, 0.0]
    # all ties: the in-grid slots in slot order, which is ascending j; a corner has exactly 4
    assert idx[0, 0].tolist() == [0, 1, 3, 4] and idx[0, 5].tolist() == [1, 2, 4, 5] and idx[0, 1].tolist() == [0, 1, 2, 3]
    assert torch.isfinite(val).all()
    assert local.max_k(grid, r) == 4 and local.max_k((1, 1), 8) == 1 and local.max_k((5, 7), 8) == 35 and local.max_k((20, 20), 2) == 9
    for bad in (5, 0, -1, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            local.topk(torch.from_numpy(c), grid, bad)
    with pytest.raises(ValueError, match="rows"):
        local.topk(torch.from_numpy(c), (3, 3), 1)
    with pytest.raises(ValueError, match="slots"):
        local.topk(torch.zeros(1, 6, 10), grid, 1)
    with pytest.raises(TypeError):
        local.topk(torch.zeros(6, 9), grid, 1)


def test_soft_displacement_on_designed_costs():
    from vdr import local
    r = 2
    c = torch.full((1, 4, 25), -INF)
    c[0, 0, 3] = 0.3                      # one finite slot: its offset, weight 1
    c[0, 1, 7] = c[0, 1, 19] = -0.2       # two equal slots: their mean
    c[0, 2, 12] = 0.9                     # the centre alone: no motion
    c[0, 3, 0] = c[0, 3, 4] = c[0, 3, 20] = c[0, 3, 24] = 0.5  # the four corners: they cancel
    flow, conf = local.soft_displacement(c, r, 0.1)
    off = lref.offsets(r)
    assert flow.dtype == torch.float32 and tuple(flow.shape) == (1, 4, 2) and tuple(conf.shape) == (1, 4)
    assert flow[0, 0].tolist() == off[3].tolist() and conf[0, 0].item() == 1.0
    assert flow[0, 1].tolist() == ((off[7] + off[19]) / 2).tolist() and conf[0, 1].item() == 0.5
    assert flow[0, 2].tolist() == [0.0, 0.0] and conf[0, 2].item() == 1.0
    assert flow[0, 3].tolist() == [0.0, 0.0] and conf[0, 3].item() == 0.25
    with pytest.raises(ValueError, match="temperature"):
        local.soft_displacement(c, r, 0.0)
    with pytest.raises(ValueError, match="slots"):
        local.soft_displacement(c, 1, 0.1)


@pytest.mark.parametrize("grid,r,temperature", (((5, 7), 2, 0.1), ((9, 17), 8, 0.07), ((3, 3), 4, 1.0)))
def test_soft_displacement_on_random_costs_stays_inside_the_bound(grid, r, temperature):
    from vdr import local
    _, ok = lref.window(grid[0], grid[1], r)
    gen = torch.Generator().manual_seed(grid[0] * 100 + r)
    c = torch.rand(2, grid[0] * grid[1], (2 * r + 1) ** 2, generator=gen) * 2 - 1  # cosines
    c = torch.where(torch.from_numpy(ok)[None], c, torch.full_like(c, -INF))
    flow, conf = local.soft_displacement(c, r, temperature)
    wf, wc = lref.soft_displacement(c, r, temperature)
    bf, bc = lref.soft_bound(c, r, temperature)
    ef, ec = np.abs(flow.numpy().astype(np.float64) - wf), np.abs(conf.numpy().astype(np.float64) - wc)
    print(f"{grid} r={r} T={temperature}: max flow error {ef.max():.3e} (bound there {bf.flat[ef.argmax()]:.3e}, max error / bound "
          f"{(ef / np.maximum(bf, 1e-300)).max():.3f}), max conf error {ec.max():.3e} (max error / bound {(ec / bc).max():.3f})")
    assert (ef <= bf).all() and (ec <= bc).all()
    assert np.abs(wf).max() <= r and (wc > 0).all() and (wc <= 1).all()


def _stub_model(cfg, grid=(2, 2), size=(32, 32), stride=16):
    from vdr.model import VitDescriptorModel
    m = VitDescriptorModel.__new__(VitDescriptorModel)
    m.cfg, m.model_name, m.dynamic_size, m.device = cfg, "stub", False, torch.device("cpu")
    m.engine = types.SimpleNamespace(grid=grid, input_size=size, patch_stride=stride)
    return m


def test_propagate_labels_refusals_need_no_device():
    import vdr
    m = _stub_model(vdr.ARCHS["vit_tiny16_224"])
    a, lab = torch.zeros(2, 3, 32, 32), torch.zeros(2, 2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="same shape"):
        m.propagate_labels(a, lab, torch.zeros(2, 3, 32, 48), 3, radius=1, k=1)
    with pytest.raises(ValueError, match="same shape"):
        m.propagate_labels(a, lab, a[:1], 3, radius=1, k=1)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.propagate_labels(a[0], lab, a[0], 3, radius=1, k=1)
    with pytest.raises(ValueError, match="input size in force"):
        m.propagate_labels(torch.zeros(2, 3, 48, 48), lab, torch.zeros(2, 3, 48, 48), 3, radius=1, k=1)
    for bad in (0, 9, -2, 1.5):
        with pytest.raises(ValueError, match="radius"):
            m.propagate_labels(a, lab, a, 3, radius=bad, k=1)
    for bad in (lab[:1], lab.reshape(2, 4), torch.zeros(2, 3, 2, dtype=torch.int64), lab.float(), lab.bool(), None):
        with pytest.raises(ValueError, match="labels_src"):
            m.propagate_labels(a, bad, a, 3, radius=1, k=1)
    for bad in (5, 0, -1, 1.5):  # a corner of the 2 x 2 grid has 4 candidates at any radius
        with pytest.raises(ValueError, match="k must be"):
            m.propagate_labels(a, lab, a, 3, radius=4, k=bad)
    for bad in (lab + 3, lab - 1):
        with pytest.raises(ValueError, match=r"0\.\.2"):
            m.propagate_labels(a, bad, a, 3, radius=1, k=1)
    with pytest.raises(ValueError, match="n_classes"):
        m.propagate_labels(a, lab, a, 0, radius=1, k=1)
    with pytest.raises(ValueError, match="temperature"):
        m.propagate_labels(a, lab, a, 3, radius=1, k=1, temperature=0.0)
    with pytest.raises(ValueError, match="facet"):
        m.propagate_labels(a, lab, a, 3, facet="keys")
    with pytest.raises(ValueError, match="hierarchy"):
        m.propagate_labels(a, lab, a, 3, bin=True, hierarchy=4)
    with pytest.raises(ValueError, match="out of range"):
        m.propagate_labels(a, lab, a, 3, layer=12)
    m.cfg = vdr.ARCHS["medsam"]
    with pytest.raises(ValueError, match="SAM"):
        m.propagate_labels(a, lab, a, 3)


def test_find_correspondences_radius_refusals_need_no_device():
    import vdr
    m = _stub_model(vdr.ARCHS["vit_tiny16_224"])
    a = torch.zeros(1, 3, 32, 32)
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError, match="radius"):
            m.find_correspondences(a, a, radius=bad)
    with pytest.raises(ValueError, match="keep_cost"):
        m.find_correspondences(a, a, keep_cost=True)
    with pytest.raises(ValueError, match="same shape"):
        m.find_correspondences(a, torch.zeros(1, 3, 32, 48), radius=2)
    m.cfg = vdr.ARCHS["siglip_base16_224"]  # no CLS token: no saliency
    with pytest.raises(ValueError, match="CLS"):
        m.find_correspondences(a, a, radius=2)


def test_displacement_is_consistent_with_nn12():
    import vdr
    gh, gw = 3, 4
    nn12 = torch.tensor([[5, 0, 11, 3, 4, 5, 6, 7, 0, 9, 10, 8]], dtype=torch.int32)
    z = torch.zeros(1, 12)
    c = vdr.Correspondences(nn12, z, nn12, z, z, z, z.bool(), (gh, gw), 8, 16)
    d = c.displacement()
    assert d.dtype == torch.int32 and tuple(d.shape) == (1, gh, gw, 2)
    assert d[0, 0, 0].tolist() == [1, 1] and d[0, 0, 1].tolist() == [0, -1] and d[0, 0, 2].tolist() == [2, 1] and d[0, 2, 0].tolist() == [-2, 0]
    i = torch.arange(12).view(1, gh, gw)
    assert torch.equal((i // gw + d[..., 0]) * gw + (i % gw + d[..., 1]), nn12.view(1, gh, gw).long())
    assert torch.equal(c.pixel_displacement(), d * 8) and c.radius is None and c.cost12 is None
