"""CPU: the k-nearest-neighbour op without a device -- vdr_op_knn / vdr_knn_work_bytes are declared, bound and exported and
refuse bad arguments before they touch a device; the index arithmetic the kernels share (csrc/knn_map.h) is walked by a host
program; vdr.knn.topk_dense / search / KnnClassifier on CPU tensors return scikit-learn's neighbours and predict_proba on
the golden files; chunked search equals the unchunked one; vdr.ops.knn refuses on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import host_program
import knn_ref as kr
import nn_cosine_ref as nref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")


def test_header_binding_and_exports_declare_the_knn_entry_points():
    import vdr
    from vdr import _lib, ops
    src = open(os.path.join(ROOT, "include", "vdr.h")).read()
    assert re.search(r"size_t vdr_knn_work_bytes\(int pairs, int tq, int tc, int k\);", src)
    assert re.search(r"int vdr_op_knn\(const void\* x, int64_t ldx, int64_t x_stride, int tq, const void\* y, int64_t ldy, "
                     r"int64_t y_stride, int tc,\s*int pairs, int d, int k, int metric, int exclude_diag, void\* work, float\* val, "
                     r"int32_t\* idx, void\* stream\);", src)
    assert "#define VDR_KNN_MAX_K 16" in src and "VDR_KNN_COSINE = 0, VDR_KNN_L2 = 1" in src
    assert {"vdr_op_knn", "vdr_knn_work_bytes"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "vdr_op_knn") and hasattr(lib, "vdr_knn_work_bytes") and lib.vdr_abi_version() == 8
    assert ops.KNN_MAX_K == 16 and ops.KNN_METRICS == ("cosine", "l2") and callable(ops.knn)
    for name in ("topk_dense", "search", "graph", "KnnClassifier", "vote", "lowest_argmax"):
        assert callable(getattr(vdr.knn, name)), name
    for name in ("transfer_labels", "fit_knn", "knn_predict", "propagate_labels"):
        assert callable(getattr(vdr.VitDescriptorModel, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^NOCONTRACT :=.*\bknn\b", mk, re.M) and re.search(r"^SRCS\s+:=.*\bknn\.hip\b", mk, re.M)


def test_op_knn_refuses_bad_arguments_before_touching_a_device():
    from vdr import _lib
    lib = _lib.load()
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 255) & ~255
    x, y, work, val, idx = (base + 1024 * k for k in range(5))

    def call(x=x, ldx=32, xs=96, tq=3, y=y, ldy=32, ys=160, tc=5, pairs=2, d=32, k=2, metric=0, diag=0, work=work, val=val, idx=idx):
        return lib.vdr_op_knn(x, ldx, xs, tq, y, ldy, ys, tc, pairs, d, k, metric, diag, work, val, idx, None)

    for kw in (dict(d=16, ldx=16, ldy=16), dict(d=48, ldx=48, ldy=48), dict(d=8), dict(d=33, ldx=40, ldy=40)):
        assert call(**kw) == -7, kw  # VDR_ERR_UNSUPPORTED
        assert lib.vdr_last_error(None).startswith(b"knn: d ")
    for k in (0, -1, 17, 20, 200):
        assert call(k=k, tc=300, ys=9600) == -7, k
        assert b"k must be 1 .. 16" in lib.vdr_last_error(None)
    invalid = [dict(x=None), dict(y=None), dict(work=None), dict(val=None), dict(idx=None),
               dict(pairs=0), dict(pairs=-1), dict(tq=0), dict(tc=-2), dict(d=0), dict(d=-32),
               dict(ldx=24), dict(ldy=31), dict(d=64), dict(xs=-96), dict(ys=-8),
               dict(x=x + 2), dict(x=x + 8), dict(y=y + 4), dict(work=work + 8), dict(val=val + 4), dict(idx=idx + 8),
               dict(ldx=36), dict(ldy=44), dict(xs=100), dict(ys=164),
               dict(metric=2), dict(metric=-1),
               dict(k=6), dict(k=5, diag=1), dict(k=16, tc=15), dict(k=1, tc=1, diag=1),
               dict(pairs=2, tq=2 ** 30), dict(pairs=3, tc=2 ** 30), dict(pairs=2 ** 16, tq=2 ** 15),
               dict(pairs=2 ** 12, tq=2 ** 16, k=16, tc=16)]  # pairs * tq * k = 2^32
    for kw in invalid:
        assert call(**kw) == -1, kw  # VDR_ERR_INVALID
        assert lib.vdr_last_error(None).startswith(b"knn: "), kw
    assert call(k=6) == -1 and b"fewer than k" in lib.vdr_last_error(None)
    assert call(metric=7) == -1 and b"metric" in lib.vdr_last_error(None)
    # the order: the operand check first, then k, then the metric, then the candidate count
    assert call(d=48, ldx=48, ldy=48, k=0, metric=9) == -7 and b"multiple of 32" in lib.vdr_last_error(None)
    assert call(k=0, metric=9) == -7 and call(k=5, metric=9) == -1 and b"metric" in lib.vdr_last_error(None)
    # well-formed calls (a stride of 0, k == tc, the diagonal excluded, l2) get as far as the device check: without a device
    # that is VDR_ERR_NO_DEVICE, after every refusal above
    for kw in (dict(), dict(ys=0), dict(k=5), dict(k=4, diag=1), dict(metric=1), dict(xs=0, ys=0)):
        rc = call(**kw)
        assert rc in (0, -2, -3), kw
        if not torch.cuda.is_available():
            assert rc == -2, kw


def test_work_bytes_is_what_the_plan_says():
    from vdr import _lib
    wb = _lib.load().vdr_knn_work_bytes
    for pairs, tq, tc, k in ((1, 1, 1, 1), (3, 300, 700, 9), (8, 3969, 3969, 16), (1, 1024, 65536, 16), (64, 196, 196, 5)):
        w = wb(pairs, tq, tc, k)
        npan, ntil = -(-tq // 128), -(-tc // 128)
        nsplit = min(max(512 // (pairs * npan), 1), ntil)
        part = -(-(pairs * nsplit * 4 * k * tq) // 4) * 4
        assert w == 4 * (pairs * 128 * (npan + ntil) + 2 * part) and w % 16 == 0, (pairs, tq, tc, k)
    assert wb(0, 5, 5, 1) == 0 and wb(1, 0, 5, 1) == 0 and wb(1, 5, -1, 1) == 0 and wb(1, 5, 5, 0) == 0 and wb(1, 5, 5, 17) == 0
    assert wb(8, 3969, 3969, 16) == 32776192  # the shape at which the earlier kernel's benchmark died, as the host walk prints it


def test_the_map_walk_finds_every_address_inside_its_extent(tmp_path):
    """tests/knn_map_cases.cpp, a host program with its own main, over the header the kernels include"""
    lines = host_program.run("knn_map_cases", tmp_path).splitlines()
    assert lines[-1] == f"cases {len(lines) - 1}" and len(lines) > 100 and all(line.startswith("ok ") for line in lines[:-1])
    for shape in ("8x3969x3969 d=768 k=16 ", "8x3969x3969 d=768 k=1 ", "64x196x196 d=768 ", "32x729x729 d=768 ", "1x3969x3969 d=768 ",
                  "1x1024x65536 d=768 ", "1x8192x8192 d=384 ", "3x300x700 d=64 k=5 ld=64/64 stride=19200/0:",
                  "3x300x700 d=64 k=5 ld=192/192 ", "4x129x129 d=96 k=8 ld=288/288 stride=0/0:", "1x1x16 d=32 ", "3x129x1 d=32 k=1 "):
        assert any(line.startswith("ok " + shape) for line in lines), shape


def _golden(name):
    z = np.load(os.path.join(HERE, "golden", name))
    return z, kr.from_bf16_bits(z["c"]), torch.from_numpy(z["labels"]), int(z["k"])


@pytest.mark.parametrize("name", ("knn_sk_300x700x64.npz", "knn_sk_d256_k16.npz"))
def test_topk_dense_and_the_classifier_return_sklearns_answers(name):
    from vdr import knn
    z, c, labels, k = _golden(name)
    for metric in kr.METRICS:
        q = kr.from_bf16_bits(z["q"] if "q" in z else z[f"q_{metric}"])
        val, idx = knn.topk_dense(q[None], c[None], k, metric)
        assert val.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(idx.shape) == (1, q.shape[0], k)
        assert np.array_equal(idx[0].numpy(), z[f"idx_{metric}"]), (name, metric)
        s = kr.scores(q[None], c[None], metric)
        got = val.numpy().astype(np.float64)
        b = np.take_along_axis(kr.bound(q[None], c[None], s, metric), idx.numpy().astype(np.int64), -1)
        err = np.abs(got - np.take_along_axis(s, idx.numpy().astype(np.int64), -1))
        print(f"{name} {metric}: max err / bound {(err / b).max():.3e}")
        assert (err <= b).all()
        clf = knn.KnnClassifier(c, labels, z[f"proba_{metric}"].shape[1], k=k, weights="uniform", metric=metric, backend="torch")
        v2, i2 = clf.kneighbors(q)
        assert torch.equal(v2, val[0]) and torch.equal(i2, idx[0])
        proba, pred = clf.predict(q)
        assert np.array_equal(proba.numpy(), z[f"proba_{metric}"].astype(np.float32)) and np.array_equal(pred.numpy(), z[f"pred_{metric}"])


@pytest.mark.parametrize("metric", kr.METRICS)
def test_topk_dense_is_the_reference_on_designed_inputs_and_chunked_search_is_unchunked_search(metric):
    """designed inputs: every fp32 evaluation is exact, so topk_dense equals knn_ref.topk bit for bit, ties included, and a
    bank cut into chunks -- ragged last chunk, a chunk shorter than k, the own row inside one chunk -- changes nothing"""
    from vdr import knn
    q, c = nref.designed(2, 129, 300, 96, seed=77)
    s = kr.scores(q, c, metric)
    for k, diag in ((1, False), (5, True), (16, False), (16, True)):
        want_val, want_idx = kr.topk(s, k, metric, diag)
        val, idx = knn.topk_dense(q, c, k, metric, diag)
        assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(val.numpy().astype(np.float64), want_val)
        for chunk in (7, 128, 299, 300, 1000):
            v, i = knn.search(q, c, k, metric=metric, exclude_diag=diag, bank_chunk=chunk)
            assert torch.equal(v, val) and torch.equal(i, idx), (k, diag, chunk)
    v, i = knn.search(q[0], c[0], 5, metric=metric)  # [tq, d] against [tc, d]
    w = knn.topk_dense(q[:1], c[:1], 5, metric)
    assert torch.equal(v, w[0][0]) and torch.equal(i, w[1][0])
    v, i = knn.search(q, c[0], 5, metric=metric)     # one bank under every query set
    w = knn.topk_dense(q, c[:1].expand(2, -1, -1), 5, metric)
    assert torch.equal(v, w[0]) and torch.equal(i, w[1])
    g = knn.graph(c[0], 4, metric=metric)
    w = knn.topk_dense(c[:1], c[:1], 4, metric, True)
    assert torch.equal(g[0], w[0][0]) and torch.equal(g[1], w[1][0]) and bool((g[1] != torch.arange(300)[:, None]).all())


def test_the_clear_shares_of_the_random_cases_are_what_the_gpu_test_asks():
    """the floors of tests/test_knn_gpu.py are on the reference alone; shown here without a device"""
    for (nq, sq), (nc, sc), d, k, floor in (((300, 11), (700, 12), 64, 5, 0.9), ((129, 21), (300, 22), 96, 8, 0.85),
                                            ((257, 31), (700, 32), 64, 16, 0.7)):
        q, c = kr.planted(nq, d, sq)[0][None], kr.planted(nc, d, sc)[0][None]
        for metric, a, diag in (("cosine", q, False), ("l2", q, False), ("cosine", c, True)):
            s = kr.scores(a, c, metric)
            share = float(kr.clear_rows(s, kr.bound(a, c, s, metric), k, metric, diag).mean())
            print(nq, nc, d, k, metric, diag, f"{share:.3f}")
            assert share >= floor


def test_knn_refuses_on_the_host_before_the_library_is_called():
    from vdr import knn, ops
    x = torch.zeros((2, 8, 32), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="HIP device"):
        ops.knn(x, x, 1)
    with pytest.raises(TypeError):
        ops.knn(x[0], x, 1)
    with pytest.raises(TypeError):
        ops.knn(x.half(), x, 1)
    for k, metric, diag, what in ((0, "cosine", False, "positive integer"), (True, "cosine", False, "positive integer"),
                                  (2.5, "cosine", False, "positive integer"), (17, "cosine", False, "out of scope"),
                                  (200, "l2", False, "out of scope"), (3, "l1", False, "metric"), (9, "cosine", False, "fewer than k"),
                                  (8, "l2", True, "fewer than k")):
        with pytest.raises(ValueError, match=what):
            ops.check_knn("knn", k, metric, 8, diag)
        with pytest.raises(ValueError, match=what):
            knn.topk_dense(x, x, k, metric, diag)
    with pytest.raises(ValueError, match="backend"):
        knn.search(x, x, 1, backend="triton")
    with pytest.raises(ValueError, match="bank_chunk"):
        knn.search(x, x, 1, bank_chunk=0)
    with pytest.raises(ValueError, match="agree"):
        knn.search(x, torch.zeros((2, 8, 64)), 1)
    with pytest.raises(ValueError, match="labels must lie"):
        knn.KnnClassifier(x[0], torch.tensor([0, 1, 2, 3, 0, 1, 2, 4]), 4, k=1)
    with pytest.raises(ValueError, match="out of scope"):
        knn.KnnClassifier(torch.zeros((300, 32)), torch.zeros(300, dtype=torch.long), 2, k=20)
