"""The vote of a row's k nearest neighbours: the second stage of the weighted k-NN classifier of frozen features (DINO /
DINOv2's evaluation beside the linear probe) and of DINO's label propagation between slices.

Plain torch: no kernel is involved, CPU and device tensors both work.  The neighbours themselves -- (value, index) lists,
best first -- come from the caller: vdr.local.topk makes them from the cost volume of a windowed correlation
(vdr.ops.local_correlation; label propagation between slices is VitDescriptorModel.propagate_labels).

The search over ALL candidates: `search` returns the k nearest bank rows of every query -- on the device by the fused top-k
kernel (vdr.ops.knn: the score matrix is never written), on the CPU or with backend="torch" by `topk_dense`, the same
definition in plain torch --, `graph` the k-NN graph of a feature matrix, and `KnnClassifier` is search + vote +
lowest_argmax: DINO's weighted k-NN classifier (weights="softmax") or scikit-learn's KNeighborsClassifier
(weights="uniform").  k is at most 16 and exactly k neighbours come back; DINO's k = 20 / 200 is out of scope.  The
definition of the scores, its float64 restatement and scikit-learn's answers on planted clusters are in tests/knn_ref.py
and tests/golden/README_knn.md."""
from __future__ import annotations

import torch

METRICS = ("cosine", "l2")
WEIGHTS = ("softmax", "uniform")


def lowest_argmax(scores: torch.Tensor) -> torch.Tensor:
    """argmax over the last dimension, the LOWEST index on a tie (torch.argmax does not promise which)"""
    C = scores.shape[-1]
    top = scores == scores.max(dim=-1, keepdim=True).values
    return torch.where(top, torch.arange(C, device=scores.device), C).min(dim=-1).values


def vote(idx: torch.Tensor, val: torch.Tensor, labels: torch.Tensor, n_classes: int, weights: str = "softmax",
         temperature: float = 0.07, metric: str = "cosine") -> torch.Tensor:
    """The neighbours' vote: idx, val [..., tq, k] -- for every query the indices of its k nearest candidates, nearest
    first, and their values (cosine similarity, or the SQUARED l2 distance with metric="l2") --, labels [..., tc] integer
    class ids of the candidates in 0..n_classes-1 (leading dimensions broadcast against idx's) -> class scores
    [..., tq, n_classes] fp32 that sum to 1 per query.
    weights="softmax": w = softmax(sim / temperature) over the k neighbours -- DINO's exp(sim / T) votes, normalised; sim is
    val for cosine and -sqrt(val) for l2; scores = (one_hot(label) * w[..., None]).sum(-2), added in neighbour order.
    weights="uniform": every neighbour counts 1 / k: scores = one_hot(label).sum(-2) / k (exact counts, one division) --
    sklearn's KNeighborsClassifier.predict_proba.
    No index_add_ and no atomics: the result is deterministic.  lowest_argmax(scores) is the predicted class, the lowest
    one on a tie."""
    if weights not in WEIGHTS:
        raise ValueError(f"vote: weights must be one of {WEIGHTS}, got {weights!r}")
    if metric not in METRICS:
        raise ValueError(f"vote: metric must be one of {METRICS}, got {metric!r}")
    if idx.dim() < 2 or idx.shape != val.shape:
        raise ValueError(f"vote: idx and val must be [..., tq, k] of one shape, got {tuple(idx.shape)} and {tuple(val.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise TypeError("vote: idx must be an integer tensor")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dim() < 1:
        raise TypeError("vote: labels must be an integer tensor [..., tc]")
    if labels.dim() > idx.dim() - 1:
        raise ValueError(f"vote: labels {tuple(labels.shape)} has more leading dimensions than idx {tuple(idx.shape)}")
    if int(n_classes) < 1:
        raise ValueError(f"vote: n_classes must be positive, got {n_classes}")
    if weights == "softmax" and not float(temperature) > 0:
        raise ValueError(f"vote: temperature must be positive, got {temperature}")
    k = idx.shape[-1]
    lab = labels.long().reshape((1,) * (idx.dim() - 1 - labels.dim()) + tuple(labels.shape))
    near = torch.take_along_dim(lab.unsqueeze(-2), idx.long(), dim=-1)         # [..., tq, k]
    hot = torch.nn.functional.one_hot(near, int(n_classes)).to(torch.float32)  # [..., tq, k, C]
    if weights == "uniform":
        return hot.sum(-2) / float(k)
    sim = val.to(torch.float32) if metric == "cosine" else -torch.sqrt(val.to(torch.float32))
    w = torch.softmax(sim / float(temperature), dim=-1)
    scores = hot[..., 0, :] * w[..., 0, None]
    for j in range(1, k):  # (the sum over the neighbours spelled out, nearest first: torch's sum() fixes no order)
        scores = scores + hot[..., j, :] * w[..., j, None]
    return scores


BACKENDS = ("auto", "kernel", "torch")


def _check_search(op: str, q, c, k, metric, exclude_diag):
    from . import ops
    for name, t in (("queries", q), ("candidates", c)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{op}: {name} must be a [P, t, d] float32 or bfloat16 tensor")
    if q.shape[0] != c.shape[0] or q.shape[2] != c.shape[2] or q.device != c.device:
        raise ValueError(f"{op}: queries {tuple(q.shape)} and candidates {tuple(c.shape)} must agree in P, d and device")
    return ops.check_knn(op, k, metric, c.shape[1], exclude_diag)


def topk_dense(q: torch.Tensor, c: torch.Tensor, k: int, metric: str = "cosine", exclude_diag: bool = False):
    """vdr.ops.knn's definition in plain torch, CPU or device: q [P, tq, d], c [P, tc, d] (fp32 is rounded once to bf16, as the
    kernel's operands are) -> (val [P, tq, k] fp32, idx [P, tq, k] int32), best first.  The [tq, tc] score matrix IS written
    here, in fp32: cosine (dot * rn(q_i)) * rn(c_j) with rn = 1 / max(sqrt(ss), 1e-8), l2 max(ss(q_i) + ss(c_j) - 2 dot, 0);
    the order is a STABLE sort of the cost (-s / s), so equal scores stay in index order.  torch's matmul fixes no summation
    order: values agree with the kernel's within the bound of tests/knn_ref.py, indices wherever no two costs are that close."""
    k = _check_search("topk_dense", q, c, k, metric, exclude_diag)
    qf, cf = q.to(torch.bfloat16).to(torch.float32), c.to(torch.bfloat16).to(torch.float32)
    dot = torch.stack([qf[p] @ cf[p].T for p in range(qf.shape[0])])  # (problem by problem: never a batched bmm)
    ssq, ssc = (qf * qf).sum(-1), (cf * cf).sum(-1)
    if metric == "cosine":
        rq, rc = 1.0 / torch.sqrt(ssq).clamp_min(1e-8), 1.0 / torch.sqrt(ssc).clamp_min(1e-8)
        s = (dot * rq[:, :, None]) * rc[:, None, :]
        cost = -s
    else:
        s = ((ssq[:, :, None] + ssc[:, None, :]) - 2.0 * dot).clamp_min(0.0)
        cost = s.clone()
    if exclude_diag:
        n = min(cost.shape[1], cost.shape[2])
        i = torch.arange(n, device=cost.device)
        cost[:, i, i] = float("inf")
    order = torch.sort(cost, dim=-1, stable=True).indices[..., :k]
    return torch.gather(s, -1, order).contiguous(), order.to(torch.int32).contiguous()


def search(q: torch.Tensor, bank: torch.Tensor, k: int, metric: str = "cosine", exclude_diag: bool = False, bank_chunk=None,
           backend: str = "auto"):
    """The k nearest rows of `bank` for every row of q: q [tq, d] with bank [tc, d], or q [P, tq, d] with bank [P, tc, d] or
    [tc, d] (one bank under every query set, at stride 0) -> (val, idx) [tq, k] / [P, tq, k], fp32 / int32, best first;
    metric, exclude_diag and the order as vdr.ops.knn's.  backend "kernel": vdr.ops.knn; "torch": topk_dense, which is also
    what CPU tensors get with "auto".  bank_chunk: a bank longer than that many rows is cut into ascending chunks; the
    chunks' lists, with their indices offset, are merged by a stable sort on the cost -- lists of ascending chunks
    concatenated are in index order among equal costs, so the result equals the unchunked call bit for bit."""
    if backend not in BACKENDS:
        raise ValueError(f"search: backend must be one of {BACKENDS}, got {backend!r}")
    if not isinstance(q, torch.Tensor) or not isinstance(bank, torch.Tensor) or q.dim() not in (2, 3) or bank.dim() not in (2, q.dim()):
        raise TypeError("search: q must be [tq, d] or [P, tq, d], bank [tc, d] or [P, tc, d]")
    flat = q.dim() == 2
    q3 = q.unsqueeze(0) if flat else q
    b3 = bank.unsqueeze(0).expand(q3.shape[0], -1, -1) if bank.dim() == 2 else bank
    k = _check_search("search", q3, b3, k, metric, exclude_diag)
    use_kernel = backend == "kernel" or (backend == "auto" and q3.is_cuda)
    if use_kernel:
        from . import ops
        one = lambda qq, c, kk, ex: ops.knn(qq, c, kk, metric, ex)
    else:
        one = lambda qq, c, kk, ex: topk_dense(qq, c, kk, metric, ex)
    tq, tc = q3.shape[1], b3.shape[1]
    if bank_chunk is not None and (isinstance(bank_chunk, bool) or int(bank_chunk) != bank_chunk or int(bank_chunk) < 1):
        raise ValueError(f"search: bank_chunk must be a positive integer, got {bank_chunk!r}")
    if bank_chunk is None or int(bank_chunk) >= tc:
        val, idx = one(q3, b3, k, exclude_diag)
    else:
        worst, none = float("-inf") if metric == "cosine" else float("inf"), 2 ** 31 - 1
        vals, idxs = [], []
        for c0 in range(0, tc, int(bank_chunk)):
            chunk = b3[:, c0:c0 + int(bank_chunk)]
            rows = chunk.shape[1]
            # a chunk's list: k places, the ones it cannot fill at the worst cost and the highest index (they sort last)
            v = torch.full((q3.shape[0], tq, k), worst, dtype=torch.float32, device=q3.device)
            i = torch.full((q3.shape[0], tq, k), none, dtype=torch.int32, device=q3.device)
            kk = min(k, rows)
            v[..., :kk], i[..., :kk] = one(q3, chunk, kk, False)
            if exclude_diag and c0 < tq:  # queries c0 .. c0 + rows - 1 have their own row in this chunk, on ITS diagonal
                q1 = min(tq, c0 + rows)
                v[:, c0:q1], i[:, c0:q1] = worst, none
                kk = min(k, rows - 1)
                if kk:
                    v[:, c0:q1, :kk], i[:, c0:q1, :kk] = one(q3[:, c0:q1], chunk, kk, True)
            vals.append(v)
            idxs.append(torch.where(i == none, i, i + c0))
        # ascending chunks concatenated are in index order among equal costs: ONE stable sort on the cost is the (cost, index) order
        v, i = torch.cat(vals, -1), torch.cat(idxs, -1)
        order = torch.sort(-v if metric == "cosine" else v, dim=-1, stable=True).indices[..., :k]
        val, idx = torch.gather(v, -1, order).contiguous(), torch.gather(i, -1, order).contiguous()
    return (val[0], idx[0]) if flat else (val, idx)


def graph(x: torch.Tensor, k: int, metric: str = "cosine", backend: str = "auto"):
    """The k-NN graph of a feature matrix x [N, d] or [P, N, d]: search(x, x, k, exclude_diag=True) -- for every row its k
    nearest OTHER rows, (val, idx) [..., N, k]; the input of a UMAP / t-SNE / spectral embedding of CLS features."""
    return search(x, x, k, metric=metric, exclude_diag=True, backend=backend)


class KnnClassifier:
    """The k-NN classifier of frozen features: features [N, d] (fp32 / bf16; kept in bf16, the kernel's operand), labels [N]
    integer classes in 0..n_classes-1.  kneighbors(q [M, d]) -> (val, idx) [M, k] by `search`; predict_proba(q) -> [M,
    n_classes] fp32 by vdr.knn.vote; predict(q) -> (scores, labels [M]) with lowest_argmax.  weights="softmax" with
    temperature 0.07 and the cosine metric is DINO's weighted k-NN evaluation (with k <= 16); weights="uniform" is
    scikit-learn's KNeighborsClassifier(algorithm="brute").predict_proba, exact counts divided once."""

    def __init__(self, features: torch.Tensor, labels: torch.Tensor, n_classes: int, k: int = 10, weights: str = "softmax",
                 temperature: float = 0.07, metric: str = "cosine", backend: str = "auto", bank_chunk=None):
        from . import ops
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("KnnClassifier: features must be a [N, d] float32 or bfloat16 tensor")
        if not isinstance(labels, torch.Tensor) or labels.dtype.is_floating_point or labels.dtype == torch.bool or \
                tuple(labels.shape) != (features.shape[0],):
            raise TypeError(f"KnnClassifier: labels must be an integer tensor of shape {(features.shape[0],)}")
        if int(n_classes) < 1 or (labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= int(n_classes))):
            raise ValueError(f"KnnClassifier: labels must lie in 0..{int(n_classes) - 1}")
        if weights not in WEIGHTS:
            raise ValueError(f"KnnClassifier: weights must be one of {WEIGHTS}, got {weights!r}")
        if weights == "softmax" and not float(temperature) > 0:
            raise ValueError(f"KnnClassifier: temperature must be positive, got {temperature}")
        if backend not in BACKENDS:
            raise ValueError(f"KnnClassifier: backend must be one of {BACKENDS}, got {backend!r}")
        self.k = ops.check_knn("KnnClassifier", k, metric, features.shape[0], False)
        self.features = features.to(torch.bfloat16).contiguous()
        self.labels = labels.to(self.features.device).long()
        self.n_classes, self.weights, self.temperature, self.metric = int(n_classes), weights, float(temperature), metric
        self.backend, self.bank_chunk = backend, bank_chunk

    def kneighbors(self, q: torch.Tensor):
        if not isinstance(q, torch.Tensor) or q.dim() != 2:
            raise TypeError("KnnClassifier: q must be a [M, d] float32 or bfloat16 tensor")
        return search(q.to(self.features.device), self.features, self.k, metric=self.metric, bank_chunk=self.bank_chunk,
                      backend=self.backend)

    def predict_proba(self, q: torch.Tensor) -> torch.Tensor:
        val, idx = self.kneighbors(q)
        return vote(idx, val, self.labels, self.n_classes, weights=self.weights, temperature=self.temperature, metric=self.metric)

    def predict(self, q: torch.Tensor):
        scores = self.predict_proba(q)
        return scores, lowest_argmax(scores)
