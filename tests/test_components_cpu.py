"""CPU: connected components without a device -- the two numpy statements (tests/components_ref.py) against scipy.ndimage.label
and the goldens it wrote (tests/golden/README_components.md); the torch statements of the kernels (vdr.components.label_torch /
clean_torch / relabel / seed_component / largest) against them; the host program over csrc/components_map.h, which runs the
kernels' own passes tile by tile in both orders under a step cap, plainly and under the sanitizers; the symbols; every refusal
of the three C entry points before the device is touched; the refusals of the Python layers."""
import ctypes as C
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

import components_ref as CR
import host_program

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")
T = CR.T


def _golden(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "components_sp_*.npz")))
    assert len(files) == 5
    for f in files:
        z = np.load(f)
        H, W = (int(v) for v in z["shape"])
        yield os.path.basename(f), z, np.unpackbits(z["mask"])[:H * W].reshape(H, W)


def _unpack(z, key, shape):
    return np.unpackbits(z[key])[:shape[0] * shape[1]].reshape(shape)


GOLDEN_CLEANS = {"holes_islands_8": dict(min_area=12, holes=True, islands=True, connectivity=8),
                 "holes_islands_4": dict(min_area=12, holes=True, islands=True, connectivity=4),
                 "islands_all_below_8": dict(min_area=100000, islands=True, connectivity=8),
                 "largest_4": dict(largest=True, connectivity=4),
                 "holes_largest_8": dict(min_area=40, holes=True, largest=True, connectivity=8)}


# ---- the numpy statements, scipy and the goldens ------------------------------------------------------------------------------------
def test_numpy_statements_equal_the_goldens_scipy_wrote(golden_dir):
    """the union-find and the breadth-first search against the stored scipy labels (first index per label = root, bincount =
    area), the restated clean rules against the stored cleaned masks"""
    for name, z, m in _golden(golden_dir):
        for conn in (4, 8):
            for value in (0, 1):
                want = CR.roots_from_labels(z[f"labels_c{conn}_v{value}"])
                assert want[2] == int(z[f"count_c{conn}_v{value}"])
                for f in (CR.roots_union_find, CR.roots_bfs):
                    got = f(m, conn, value)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, conn, value, f.__name__)
                assert np.array_equal(CR.labels_from_roots(want[0]), z[f"labels_c{conn}_v{value}"])   # scipy numbers by first pixel
        for cname, kw in GOLDEN_CLEANS.items():
            for f in (CR.roots_union_find, CR.roots_bfs):
                out, changed, stats = CR.clean(m, roots=f, **kw)
                assert np.array_equal(out, _unpack(z, f"clean_{cname}", m.shape)), (name, cname)
                assert changed == int(z[f"clean_{cname}_changed"]) and np.array_equal(stats, z[f"clean_{cname}_stats"]), (name, cname)


@pytest.mark.parametrize("H,W", [(1, 1), (2, T), (T - 1, T + 1), (T + 1, 2 * T + 1), (37, 53)])
def test_numpy_statements_equal_scipy_on_designed_and_random_planes(H, W):
    pytest.importorskip("scipy")
    planes = dict(CR.designed(H, W))
    for p in (0.1, 0.41, 0.59, 0.9):
        planes[f"bernoulli{p}"] = CR.bernoulli(H, W, p, 3 + H)
    for name, m in planes.items():
        for conn in (4, 8):
            for value in (0, 1):
                want = CR.scipy_roots(m, conn, value)
                for f in (CR.roots_union_find, CR.roots_bfs):
                    got = f(m, conn, value)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, conn, value)


# ---- the torch statements -----------------------------------------------------------------------------------------------------------
def test_torch_statements_equal_the_goldens(golden_dir):
    from vdr import components as cc
    for name, z, m in _golden(golden_dir):
        t = torch.from_numpy(m)
        for conn in (4, 8):
            for value in (0, 1):
                want = CR.roots_from_labels(z[f"labels_c{conn}_v{value}"])
                root, area, count = cc.label_torch(t, conn, value)
                assert root.dtype == area.dtype == count.dtype == torch.int32 and tuple(root.shape) == m.shape
                assert np.array_equal(root.numpy(), want[0]) and np.array_equal(area.numpy(), want[1]) and count.tolist() == [want[2]]
                assert np.array_equal(cc.relabel(root).numpy(), z[f"labels_c{conn}_v{value}"])    # scipy's numbering
        for cname, kw in GOLDEN_CLEANS.items():
            out, changed, stats = cc.clean_torch(t.bool(), **kw)
            assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), _unpack(z, f"clean_{cname}", m.shape)), (name, cname)
            assert changed.tolist() == [int(z[f"clean_{cname}_changed"])] and np.array_equal(stats[0].numpy(), z[f"clean_{cname}_stats"])


def test_torch_statements_on_a_batch_of_designed_planes():
    """a batch equals its planes one by one; seed_component and largest on the root planes; relabel of a batch"""
    from vdr import components as cc
    H, W = T + 3, T + 9
    planes = CR.designed(H, W)
    stack = torch.from_numpy(np.stack(list(planes.values())))
    for conn in (4, 8):
        root, area, count = cc.label_torch(stack, conn, 1)
        for k, (name, m) in enumerate(planes.items()):
            want = CR.roots_bfs(m, conn, 1)
            assert np.array_equal(root[k].numpy(), want[0]) and np.array_equal(area[k].numpy(), want[1]) and int(count[k]) == want[2], (name, conn)
            assert np.array_equal(cc.relabel(root)[k].numpy(), CR.labels_from_roots(want[0]))
        big = cc.largest(root, area)
        for k, (name, m) in enumerate(planes.items()):
            want = CR.clean(m, largest=True, connectivity=conn)[0]
            assert np.array_equal(big[k].numpy().astype(np.uint8), want), (name, conn)
        for kw in (dict(min_area=9, holes=True, islands=True), dict(min_area=50, holes=True, largest=True), dict()):
            out, changed, stats = cc.clean_torch(stack, connectivity=conn, **kw)
            for k, (name, m) in enumerate(planes.items()):
                want = CR.clean(m, connectivity=conn, **kw)
                assert np.array_equal(out[k].numpy(), want[0]) and int(changed[k]) == want[1] and np.array_equal(stats[k].numpy(), want[2]), (name, conn, kw)
    k = list(planes).index("equal_areas")
    root, area, _ = cc.label_torch(stack, 4, 1)
    seeds = torch.zeros(stack.shape[0], dtype=torch.int64)
    seeds[k] = (H - 1) * W + 1                                             # inside the bottom-left square
    comp = cc.seed_component(root, seeds)
    assert comp.dtype == torch.bool and int(comp[k].sum()) == 4 and bool(comp[k, H - 2:, :2].all())
    assert int(comp[list(planes).index("empty")].sum()) == 0               # a seed that is not selected: nothing
    assert int(cc.largest_root(area)[k]) == W - 2 and int(cc.largest_root(area)[list(planes).index("empty")]) == -1


# ---- the host program ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_kernels_passes_run_on_the_host_in_both_orders(tmp_path, sanitize):
    """tests/components_map_cases.cpp, a host program with its own main, over the header the kernels include: tiles own every pixel
    once, the seam pass enumerates every straddling pair, every index stays in bounds, and the passes themselves, run tile by
    tile forward and reversed under a step cap, give the breadth-first search's roots and areas; the second build runs it under
    the address and undefined-behaviour sanitizers (host code, stand-alone)"""
    out = host_program.run("components_map_cases", tmp_path, sanitize)
    lines = out.splitlines()
    assert lines[-1] == "cases 38 fails 0" and "FAIL" not in out
    assert sum(ln.endswith(" fails 0") and ln.startswith("H ") for ln in lines) == 38
    assert any(ln.startswith("H 300 W 517: tiles 45 seam items 4468 chunks 38 ") for ln in lines)
    assert any(ln.startswith(f"H {2 * T + 1} W {2 * T + 1}: tiles 9 ") for ln in lines) and any(ln.startswith("H 1 W 1: tiles 1 seam items 0 ") for ln in lines)


# ---- the C side ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_listed_in_the_makefile():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    lib = _lib.load()
    for name in ("vdr_op_mask_binarize", "vdr_op_connected_components", "vdr_op_mask_clean"):
        assert re.search(r"\bint " + name + r"\(", src) and name in _lib.SYMBOLS and hasattr(lib, name), name
    for name in ("vdr_mask_binarize_workspace_bytes", "vdr_connected_components_workspace_bytes", "vdr_mask_clean_workspace_bytes"):
        assert re.search(r"\bsize_t " + name + r"\(", src) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.vdr_abi_version() == 8 and "#define VDR_ABI_VERSION 8" in src               # additive: the version stays
    assert all(f"#define VDR_CLEAN_{n} {v}" in src for n, v in (("HOLES", 1), ("ISLANDS", 2), ("LARGEST", 4)))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^NOCONTRACT :=.*\bcomponents\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\bcomponents\.hip\b", mk, re.M)
    assert re.search(r"^ASM :=.*\bcomponents\b", mk, re.M) and "components_map.h" in mk
    assert callable(ops.mask_binarize) and callable(ops.connected_components) and callable(ops.mask_clean)
    assert hasattr(vdr, "components") and hasattr(vdr.Segmentation, "clean") and hasattr(vdr.VolumeSegmentation, "clean")
    assert vdr.segment.MaskDecoder.LAUNCHES == 52
    # 4 bytes a pixel to label; 8 a pixel, 16 a plane (rounded to 8) and 64 per 4096 pixels of a plane to clean
    assert lib.vdr_connected_components_workspace_bytes(3, 300, 517) == 4 * 3 * 300 * 517
    assert lib.vdr_mask_clean_workspace_bytes(3, 300, 517) == 8 * 3 * 300 * 517 + 8 * 3 + 8 * 2 + 64 * 3 * 38
    assert lib.vdr_mask_clean_workspace_bytes(64, 1024, 1024) <= (8 + 1 / 64) * 64 * 1024 * 1024 + 16 * 64
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 4097)):
        assert lib.vdr_connected_components_workspace_bytes(*bad) == 0 and lib.vdr_mask_clean_workspace_bytes(*bad) == 0
    assert lib.vdr_mask_binarize_workspace_bytes(2, 8, 8, 32, 32) == 16 and lib.vdr_mask_binarize_workspace_bytes(2, 257, 8, 32, 32) == 0
    # the kernels' file owns the integer atomics and says why; no other kernel source has any
    text = open(os.path.join(CSRC, "components.hip")).read()
    assert "INTEGER ATOMICS live in this file and only here" in text
    for f in glob.glob(os.path.join(CSRC, "*.hip")):
        if os.path.basename(f) != "components.hip":
            assert not re.search(r"\batomic(Add|Min|Max|CAS|Or)\b|__hip_atomic_fetch", open(f).read()), f


def test_the_three_entry_points_refuse_before_the_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 65536)()
    base = (C.addressof(raw) + 255) & ~255
    mk, ws, rt, ar, ct, ou, ch, st, lg = (base + 4096 * i for i in range(9))

    def cc(mask=mk, P=2, H=8, W=8, conn=8, value=1, work=ws, nbytes=4096, root=rt, area=ar, count=ct):
        return lib.vdr_op_connected_components(mask, P, H, W, conn, value, work, nbytes, root, area, count, None)
    for kw in (dict(mask=None), dict(work=None), dict(root=None), dict(area=None), dict(count=None), dict(P=0), dict(P=65536), dict(H=0), dict(H=4097),
               dict(W=0), dict(W=4097), dict(conn=5), dict(conn=0), dict(value=2), dict(value=-1), dict(work=ws + 8), dict(root=rt + 2), dict(area=ar + 1),
               dict(count=ct + 3)):
        assert cc(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_connected_components: "), kw
    need = lib.vdr_connected_components_workspace_bytes(2, 8, 8)
    assert need == 512 and cc(nbytes=need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_connected_components: workspace too small")

    def cl(mask=mk, P=2, H=8, W=8, min_area=3, conn=8, mode=3, work=ws, nbytes=4096, out=ou, changed=ch, stats=st):
        return lib.vdr_op_mask_clean(mask, P, H, W, min_area, conn, mode, work, nbytes, out, changed, stats, None)
    for kw in (dict(mask=None), dict(work=None), dict(out=None), dict(changed=None), dict(stats=None), dict(P=0), dict(P=65536), dict(H=0), dict(H=4097),
               dict(W=0), dict(W=4097), dict(conn=5), dict(min_area=-1), dict(mode=6), dict(mode=7), dict(mode=8), dict(mode=-1), dict(out=mk),
               dict(out=mk + 127), dict(mask=ou + 64), dict(work=ws + 8), dict(changed=ch + 2), dict(stats=st + 1)):
        assert cl(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_mask_clean: "), kw
    need = lib.vdr_mask_clean_workspace_bytes(2, 8, 8)
    assert need == 1024 + 16 + 8 + 128 and cl(nbytes=need - 1) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_mask_clean: workspace too small")
    assert cl(out=mk + 128, nbytes=need - 1) == -5                                           # exactly behind the mask: no overlap, so the workspace check is what stops it

    def bn(logits=lg, ps=64, ppg=1, gs=256, P=2, H=8, W=8, oh=32, ow=32, thr=0.0, work=ws, nbytes=16, out=ou):
        return lib.vdr_op_mask_binarize(logits, ps, ppg, gs, P, H, W, oh, ow, thr, work, nbytes, out, None)
    for kw in (dict(logits=None), dict(work=None), dict(out=None), dict(logits=lg + 2), dict(H=0), dict(H=257), dict(W=0), dict(W=257), dict(oh=0),
               dict(oh=4097), dict(ow=0), dict(ow=4097), dict(P=0), dict(P=65536), dict(ps=63), dict(thr=float("nan")), dict(ppg=0), dict(P=3, ppg=2),
               dict(P=4, ppg=2, gs=127)):
        assert bn(**kw) == -1, kw
        assert lib.vdr_last_error(None).startswith(b"vdr_op_mask_binarize: "), kw
    assert bn(nbytes=15) == -5 and lib.vdr_last_error(None).startswith(b"vdr_op_mask_binarize: workspace too small")
    if not torch.cuda.is_available():
        assert cc() == -2 and cl() == -2 and cl(mode=0) == -2 and bn() == -2                 # VDR_ERR_NO_DEVICE, after every refusal above


# ---- the Python side ----------------------------------------------------------------------------------------------------------------
def test_ops_refuse_before_any_device_work():
    from vdr import ops
    m = torch.zeros((2, 8, 8), dtype=torch.uint8)
    for bad in (torch.zeros((8, 8)), torch.zeros((1, 2, 8, 8), dtype=torch.bool), torch.zeros(8, dtype=torch.uint8), np.zeros((8, 8), np.uint8),
                torch.zeros((2, 0, 8), dtype=torch.uint8), torch.zeros((1, 4097), dtype=torch.bool)):
        with pytest.raises(ValueError, match="connected_components"):
            ops.connected_components(bad)
        with pytest.raises(ValueError, match="mask_clean"):
            ops.mask_clean(bad)
    with pytest.raises(ValueError, match="HIP device"):
        ops.connected_components(m)
    with pytest.raises(ValueError, match="HIP device"):
        ops.mask_clean(m.bool())
    for kw in (dict(connectivity=5), dict(connectivity=True), dict(value=2), dict(value=True)):
        with pytest.raises(ValueError, match="connected_components"):
            ops.connected_components(m, **kw)
    for kw in (dict(min_area=-1), dict(min_area=2.5), dict(min_area=True), dict(islands=True, largest=True), dict(connectivity=6)):
        with pytest.raises(ValueError, match="mask_clean"):
            ops.mask_clean(m, **kw)
    with pytest.raises(ValueError, match="mask_binarize"):
        ops.mask_binarize(torch.zeros((1, 8, 8)), (32, 32))                                 # not on the device
    with pytest.raises(ValueError, match="mask_binarize"):
        ops.mask_binarize(torch.zeros((1, 8, 8), dtype=torch.float64), (32, 32))


class _Cfg:
    window, img, patch = 14, 128, 16


def _handle():
    h = types.SimpleNamespace(model_name="medsam", device="cpu", cfg=_Cfg(), has_mask_decoder=True)
    h.mask_decoder = types.SimpleNamespace(g=8, has_point_prompts=True, has_mask_prompt=True)
    return h


def test_the_layers_above_refuse_before_any_device_work():
    import vdr
    from vdr import pipeline, spectral
    seg = vdr.Segmentation(torch.zeros((1, 2, 1, 32, 32)), torch.zeros((1, 2, 1)), (128, 128))
    vol = vdr.VolumeSegmentation(torch.zeros((3, 32, 32)), torch.zeros(3), torch.zeros((3, 4)), torch.zeros(3, dtype=torch.int32), (128, 128))
    for obj in (seg, vol):
        for kw in (dict(min_area=-1), dict(min_area=1.5), dict(islands=True, largest=True), dict(connectivity=3), dict(size=(0, 8)), dict(size=(8, 4097)),
                   dict(threshold=float("nan")), dict(max_planes=0)):
            with pytest.raises(ValueError, match="clean"):
                obj.clean(**kw)
    gen = vdr.VitDescriptorModel.generate_masks
    x = torch.zeros((1, 3, 128, 128))
    for bad in (-1, 2.5, True, "many"):
        with pytest.raises(ValueError, match="min_mask_region_area"):
            gen(_handle(), x, min_mask_region_area=bad)
    lg = torch.full((2, 4, 4), -1.0)
    ms = vdr.MaskSet(lg, torch.ones(2), torch.ones(2), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 2)),
                     torch.arange(2), torch.zeros(2, dtype=torch.int64), (16, 16), (4, 4), 0.0, cleaned=torch.ones((2, 4, 4), dtype=torch.uint8),
                     changed=torch.zeros(2, dtype=torch.int32))
    assert bool(ms.masks().all()) and ms.masks().dtype == torch.bool and ms.label_map().tolist() == [[2] * 4] * 4   # the cleaned planes, not the logits
    assert [r["counts"] for r in ms.rle()] == [[0, 16], [0, 16]]
    with pytest.raises(ValueError, match="cleaned"):
        ms.masks((8, 8))
    for f in (pipeline.segment_volume, pipeline.propagate_segmentation):
        for kw in (dict(min_region_area=-1), dict(min_region_area=1.5), dict(fill_holes=True), dict(min_region_area=4, keep_largest="yes")):
            with pytest.raises(ValueError, match="min_region_area|fill_holes|keep_largest"):
                f(None, None, None, **kw) if f is pipeline.segment_volume else f(None, None, None, None, **kw)
    bits = torch.zeros((1, 16, 1), dtype=torch.int32)
    with pytest.raises(ValueError, match="labelling"):
        spectral.tokencut(bits, (4, 4), labelling="gpu")
    with pytest.raises(ValueError, match="labelling"):
        spectral.lost(bits, (4, 4), labelling="gpu")
