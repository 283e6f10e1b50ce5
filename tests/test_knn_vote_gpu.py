"""GPU: vdr.knn.vote on device tensors -- the CPU result (bitwise for uniform weights, where every step is exact or one
division; within fp32 rounding of exp for softmax), the same bits from run to run, and batch independence."""
import os

import numpy as np
import pytest
import torch

import knn_ref as kref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("metric", kref.METRICS)
def test_vote_on_the_device_equals_sklearn_and_the_cpu(metric):
    import vdr
    g = np.load(os.path.join(GOLDEN, "knn_sk_300x700x64.npz"))
    q, c, k = kref.from_bf16_bits(g["q"]), kref.from_bf16_bits(g["c"]), int(g["k"])
    idx = torch.from_numpy(g[f"idx_{metric}"])
    val = torch.from_numpy(kref.topk(kref.scores(q[None], c[None], metric), k, metric)[0][0]).float()
    labels = torch.from_numpy(g["labels"])
    uni = vdr.knn.vote(idx.cuda(), val.cuda(), labels.cuda(), 7, weights="uniform", metric=metric)
    assert uni.is_cuda and uni.dtype == torch.float32
    assert np.array_equal(uni.cpu().numpy(), g[f"proba_{metric}"].astype(np.float32))
    assert np.array_equal(vdr.knn.lowest_argmax(uni).cpu().numpy(), g[f"pred_{metric}"])
    soft = vdr.knn.vote(idx.cuda(), val.cuda(), labels.cuda(), 7, metric=metric)
    assert torch.equal(soft, vdr.knn.vote(idx.cuda(), val.cuda(), labels.cuda(), 7, metric=metric))
    cpu = vdr.knn.vote(idx, val, labels, 7, metric=metric)
    # softmax weights lie in [0, 1]: exp and the division differ by a few ulp of 1 between the two back ends, k = 5 terms
    assert (soft.cpu() - cpu).abs().max() <= 16 * 2.0 ** -24
    assert torch.allclose(soft.sum(-1), torch.ones(300, device="cuda"), atol=1e-6)
    # int32 indices (what a kernel writes) and a batch: a problem's scores do not depend on its position
    b3 = vdr.knn.vote(idx.int().cuda().expand(3, 300, k), val.cuda().expand(3, 300, k), labels.cuda(), 7, metric=metric)
    assert torch.equal(b3[0], soft) and torch.equal(b3[2], soft)
