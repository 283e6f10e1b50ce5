"""The vote of a row's k nearest neighbours: the second stage of the weighted k-NN classifier of frozen features (DINO /
DINOv2's evaluation beside the linear probe) and of DINO's label propagation between slices.

Plain torch: no kernel is involved, CPU and device tensors both work.  The neighbours themselves -- (value, index) lists,
best first -- come from the caller: vdr.local.topk makes them from the cost volume of a windowed correlation
(vdr.ops.local_correlation; label propagation between slices is VitDescriptorModel.propagate_labels); for a search over ALL
candidates this library has a top-1 kernel (vdr.ops.nn_cosine) and no top-k kernel yet.  The
definition of the scores such a kernel has to return, its float64 restatement and scikit-learn's answers on planted
clusters are in tests/knn_ref.py and tests/golden/README_knn.md."""
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
