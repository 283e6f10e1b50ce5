"""Lloyd's k-means of dense descriptor maps on the device: the assignment and the update step are libvdr.so kernels
(vdr.ops.kmeans_assign / kmeans_update, csrc/kmeans.hip); the loop, the initialisations and the restarts are here.  `vote`
is the saliency vote of the co-segmentation (pure torch, CPU tensors work too)."""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import torch

from . import ops

INITS = ("maximin", "first", "random")


class ConvergenceWarning(UserWarning):
    """fit: some problems were still changing labels after max_iter iterations (KMeans.converged is False for them)"""


@dataclass
class KMeans:
    """A fitted k-means of `problems` problems (one per image, or one for all images when fitted with joint=True), R rows
    each.  labels [problems, R] int32; centroids [problems, k, d] fp32, the means of the final labels (an empty cluster
    keeps the centroid it had); inertia [problems] fp32, the sum of squared distances of the last assignment; counts
    [problems, k] int32; iters [problems] int32, the assign + update iterations run, the one that changed no label
    included (sklearn's n_iter_); converged [problems] bool."""
    labels: torch.Tensor
    centroids: torch.Tensor
    inertia: torch.Tensor
    counts: torch.Tensor
    iters: torch.Tensor
    converged: torch.Tensor

    @property
    def k(self) -> int:
        return int(self.centroids.shape[1])


def _first_index(mask: torch.Tensor) -> torch.Tensor:
    """mask [..., n] bool with at least one True per row -> the lowest True index [...]"""
    n = mask.shape[-1]
    return torch.where(mask, torch.arange(n, device=mask.device), n).min(dim=-1).values


def maximin(x: torch.Tensor, k: int) -> torch.Tensor:
    """Deterministic farthest-point initialisation: x [problems, R, d] (any float dtype, any device) -> the indices
    [problems, k] int64 of the chosen rows.  The first is the row of largest squared norm; each next one the row whose
    squared distance to the nearest chosen row is largest; ties go to the lowest index.  float64 arithmetic in plain
    torch."""
    xf = x.to(torch.float64)
    idx = torch.empty((xf.shape[0], k), dtype=torch.int64, device=xf.device)
    sq = (xf * xf).sum(-1)
    cur = _first_index(sq == sq.max(dim=-1, keepdim=True).values)
    mind = torch.full_like(sq, float("inf"))
    for j in range(k):
        idx[:, j] = cur
        c = torch.gather(xf, 1, cur.view(-1, 1, 1).expand(-1, 1, xf.shape[2]))
        mind = torch.minimum(mind, ((xf - c) ** 2).sum(-1))
        cur = _first_index(mind == mind.max(dim=-1, keepdim=True).values)
    return idx


def vote(labels: torch.Tensor, saliency: torch.Tensor, k: int, thresh: float = 0.065, votes_percentage: float = 75) -> torch.Tensor:
    """The saliency vote of the co-segmentation: labels [B, n] (integers in 0..k-1), saliency [B, n] -> salient [k] bool.  An
    image votes for a cluster when the mean saliency (float64) of its patches in the cluster exceeds `thresh`; an image
    with no patch in the cluster votes no.  A cluster is salient when at least votes_percentage % of the B images vote
    for it.  Pure torch on the tensors' device."""
    if labels.dim() != 2 or labels.shape != saliency.shape:
        raise ValueError(f"vote: labels [B, n] and saliency [B, n] expected, got {tuple(labels.shape)} and {tuple(saliency.shape)}")
    if k < 1:
        raise ValueError(f"vote: k must be positive, got {k}")
    B = labels.shape[0]
    onehot = labels.long().unsqueeze(-1) == torch.arange(k, device=labels.device)  # [B, n, k]
    cnt = onehot.sum(1)
    ssum = (onehot * saliency.to(torch.float64).unsqueeze(-1)).sum(1)
    mean = ssum / cnt.clamp_min(1)
    votes = ((cnt > 0) & (mean > thresh)).sum(0)
    return votes.double() * 100.0 >= float(votes_percentage) * B


def _rows(o: ops.KmeansOperand) -> torch.Tensor:
    """the operand's rows as a [problems, R, d] bf16 tensor (a view where it can be)"""
    x = o.x
    return x.reshape(x.shape[0], o.R, o.d)


def _init_centroids(o: ops.KmeansOperand, k: int, init, gen) -> torch.Tensor:
    if isinstance(init, torch.Tensor):
        if init.dim() != 3 or tuple(init.shape) != (o.problems, k, o.d):
            raise ValueError(f"kmeans.fit: an init tensor must have shape ({o.problems}, {k}, {o.d}), got {tuple(init.shape)}")
        return init.to(device=o.x.device, dtype=torch.float32).contiguous().clone()
    rows = _rows(o)
    if init == "maximin":
        idx = maximin(rows[:1] if o.problem_stride == 0 and o.problems > 1 else rows, k).expand(o.problems, k)
    elif init == "first":
        idx = torch.arange(k, device=rows.device).expand(o.problems, k)
    else:
        idx = torch.stack([torch.randperm(o.R, generator=gen)[:k] for _ in range(o.problems)]).to(rows.device)
    return torch.gather(rows, 1, idx.unsqueeze(-1).expand(-1, -1, o.d)).to(torch.float32).contiguous()


def _lloyd(o: ops.KmeansOperand, cent: torch.Tensor, max_iter: int, sync_every: int) -> KMeans:
    """the loop on one operand: enqueued without host synchronisation, every launch returns at once for a finished problem"""
    dev, k = o.x.device, int(cent.shape[1])
    work = o.work(k)
    labels = torch.full((o.problems, o.R), -1, dtype=torch.int32, device=dev)
    min_dist = torch.empty((o.problems, o.R), dtype=torch.float32, device=dev)
    inertia = torch.empty((o.problems,), dtype=torch.float32, device=dev)
    changed = torch.ones((o.problems,), dtype=torch.int32, device=dev)  # doubles as the `active` flag of the next launches
    counts = torch.zeros((o.problems, k), dtype=torch.int32, device=dev)
    iters = torch.zeros((o.problems,), dtype=torch.int32, device=dev)
    for it in range(max_iter):
        iters += changed.ne(0)
        ops.kmeans_assign(o, cent, labels, active=changed, out=(min_dist, inertia, changed), work=work)
        ops.kmeans_update(o, labels, cent, active=changed, inplace=True, counts=counts, work=work)
        if sync_every and (it + 1) % sync_every == 0 and not bool(changed.any()):
            break
    return KMeans(labels, cent, inertia, counts, iters, changed.eq(0))


def _check_fit(x, k, init, n_init, max_iter, sync_every):
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("kmeans.fit: x must be a [P, t, d] or [t, d] float32 or bfloat16 tensor")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.KMEANS_MAX_K:
        raise ValueError(f"kmeans.fit: k must be an integer in 1..{ops.KMEANS_MAX_K}, got {k!r}")
    if not isinstance(init, torch.Tensor) and init not in INITS:
        raise ValueError(f"kmeans.fit: init must be one of {INITS} or a [problems, k, d] tensor, got {init!r}")
    if n_init < 1 or (n_init > 1 and (isinstance(init, torch.Tensor) or init != "random")):
        raise ValueError("kmeans.fit: n_init must be >= 1, and n_init > 1 goes with init='random' only (the other "
                         "initialisations are deterministic)")
    if max_iter < 1 or sync_every < 0:
        raise ValueError("kmeans.fit: max_iter must be >= 1, sync_every >= 0")
    if x.shape[-1] % 32:
        raise ValueError(f"kmeans.fit: d must be a multiple of 32, got {x.shape[-1]}")


def fit(x: torch.Tensor, k: int, init="maximin", n_init: int = 1, max_iter: int = 300, joint: bool = False,
        sync_every: int = 16, seed: int = 0) -> KMeans:
    """Lloyd's k-means of descriptor maps x [P, t, d] (or one map [t, d]) bf16 / fp32 on the device: per image, or of all
    P * t rows together with joint=True.  fp32 maps are rounded once to bf16.  1 <= k <= min(1024, rows), d % 32 == 0.
    Iterations of assign + update run until an assign changes no label of the problem (sklearn's fixed point at tol=0), at
    most max_iter; the centroids returned are the means of the final labels.  The loop is enqueued without host
    synchronisation; after every sync_every iterations one read of the flags ends it early.  sync_every=0 never reads them
    (nothing in the loop waits for the device, which is what a graph capture of it needs; no ConvergenceWarning is raised
    then, `converged` tells) -- the result's bits are the same either way.
    init: "maximin" (deterministic farthest point, see maximin), "first" (rows 0..k-1), "random" (k distinct rows drawn with
    a torch generator seeded with `seed`) or a [problems, k, d] tensor taken as given.  n_init > 1 (init="random"): the
    restart of lowest inertia per problem is kept, the lowest restart index on a tie; over one map (or a joint fit) the
    restarts run as extra problems over the same rows (a problem stride of 0)."""
    _check_fit(x, k, init, n_init, max_iter, sync_every)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    rows = x.shape[0] * x.shape[1] if joint else x.shape[1]
    if k > rows:
        raise ValueError(f"kmeans.fit: k = {k} exceeds the {rows} rows of a problem")
    o = ops.kmeans_operand(x, joint, "kmeans.fit")
    gen = torch.Generator().manual_seed(int(seed)) if isinstance(init, str) and init == "random" else None
    if n_init == 1:
        runs = [_lloyd(o, _init_centroids(o, k, init, gen), max_iter, sync_every)]
    elif o.problems == 1:
        on = ops.kmeans_operand(o.x.expand(n_init, o.imgs, o.t, o.d), False, "kmeans.fit")
        r = _lloyd(on, _init_centroids(on, k, init, gen), max_iter, sync_every)
        runs = [KMeans(*(getattr(r, f)[i:i + 1] for f in ("labels", "centroids", "inertia", "counts", "iters", "converged")))
                for i in range(n_init)]
    else:
        runs = [_lloyd(o, _init_centroids(o, k, init, gen), max_iter, sync_every) for _ in range(n_init)]
    if len(runs) == 1:
        res = runs[0]
    else:
        inertia = torch.stack([r.inertia for r in runs])  # [n_init, problems]
        best = _first_index((inertia == inertia.min(dim=0, keepdim=True).values).t())  # [problems]
        pick = lambda f: torch.stack([getattr(r, f) for r in runs])[best, torch.arange(o.problems, device=best.device)]  # noqa: E731
        res = KMeans(pick("labels"), pick("centroids"), pick("inertia"), pick("counts"), pick("iters"), pick("converged"))
    if sync_every and not bool(res.converged.all()):
        n_bad = int((~res.converged).sum())
        warnings.warn(f"kmeans.fit: {n_bad} of {o.problems if n_init == 1 or o.problems > 1 else 1} problems were still changing "
                      f"labels after {max_iter} iterations", ConvergenceWarning, stacklevel=2)
    return res


def elbow(x: torch.Tensor, k_max: int = 14, ratio: float = 0.975, **fit_kwargs) -> KMeans:
    """Fits k = 1, 2, ..., k_max and returns the first fit whose mean inertia (summed over the problems, per row) exceeds
    `ratio` times the previous one -- the fit at k_max (or at a problem's row count, when that is smaller) when none does.
    One host read per k."""
    if k_max < 1:
        raise ValueError(f"kmeans.elbow: k_max must be positive, got {k_max}")
    prev, res = None, None
    if isinstance(x, torch.Tensor) and x.dim() in (2, 3):  # (a map with fewer than k_max rows: the sweep ends at its row count)
        k_max = min(k_max, x.shape[-2] * (x.shape[0] if x.dim() == 3 and fit_kwargs.get("joint") else 1))
    for k in range(1, k_max + 1):
        res = fit(x, k, **fit_kwargs)
        mean = float(res.inertia.double().sum()) / float(res.labels.numel())
        if prev is not None and mean > ratio * prev:
            break
        prev = mean
    return res
