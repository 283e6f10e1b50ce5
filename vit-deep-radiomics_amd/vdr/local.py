"""What is done with the cost volume of a windowed correlation (vdr.ops.local_correlation, csrc/local_corr.hip): the k best
candidates of every patch inside its window -- the (idx, val) lists vdr.knn.vote takes, which is DINO's label propagation
between slices --, a soft displacement field, and vote_window: the multi-source soft vote of vdr.ops.window_vote
(csrc/window_vote.hip) restated in torch, which is what VitDescriptorModel.propagate_volume's kernel is read against.

Plain torch: no kernel is involved, CPU and device tensors both work.  A cost volume is [P, t, W * W] fp32 on a gh x gw grid,
t = gh * gw, W = 2 * radius + 1; slot (dy + radius) * W + (dx + radius) of row i = qy * gw + qx holds the similarity of patch
i and the candidate at (qy + dy, qx + dx), -inf where that is outside the grid (include/vdr.h)."""
from __future__ import annotations

import torch

from .ops import LOCAL_CORR_MAX_RADIUS, check_local_radius


def _radius_of(cost: torch.Tensor, op: str) -> int:
    if not isinstance(cost, torch.Tensor) or cost.dim() != 3 or not cost.dtype.is_floating_point:
        raise TypeError(f"{op}: cost must be a [P, t, W * W] floating-point tensor")
    for r in range(1, LOCAL_CORR_MAX_RADIUS + 1):
        if (2 * r + 1) ** 2 == cost.shape[2]:
            return r
    raise ValueError(f"{op}: cost has {cost.shape[2]} slots, which is (2 r + 1)^2 for no radius in 1..{LOCAL_CORR_MAX_RADIUS}")


def offsets(radius: int, device=None) -> torch.Tensor:
    """[W * W, 2] int64: the displacement (dy, dx) of every slot of a window of `radius`, in slot order"""
    r = check_local_radius("offsets", radius)
    W = 2 * r + 1
    w = torch.arange(W * W, device=device)
    return torch.stack((torch.div(w, W, rounding_mode="floor") - r, w % W - r), dim=1)


def max_k(grid, radius: int) -> int:
    """The smallest number of in-grid slots any patch of the grid has -- a corner's: min(gh, r + 1) * min(gw, r + 1)"""
    gh, gw = (int(v) for v in grid)
    return min(gh, radius + 1) * min(gw, radius + 1)


def topk(cost: torch.Tensor, grid, k: int):
    """The k best candidates of every patch inside its window: cost [P, t, W * W] on grid = (gh, gw) -> (idx [P, t, k] int32,
    the candidates' indices j = (qy + dy) * gw + (qx + dx) into the other map; val [P, t, k] fp32, their similarities), best
    first, equal values in slot order (a stable descending sort: the lowest slot, which is the lowest j, first).  k above
    max_k(grid, radius) is refused: a corner patch has no more candidates, and a -inf slot is never returned.  The output
    is what vdr.knn.vote takes."""
    r = _radius_of(cost, "topk")
    gh, gw = (int(v) for v in grid)
    if gh <= 0 or gw <= 0 or gh * gw != cost.shape[1]:
        raise ValueError(f"topk: cost has {cost.shape[1]} rows, the grid {gh} x {gw}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= max_k((gh, gw), r):
        raise ValueError(f"topk: k must be 1..{max_k((gh, gw), r)} (the in-grid candidates of a corner patch of a {gh} x {gw} grid "
                         f"at radius {r}), got {k!r}")
    k = int(k)
    order = torch.sort(cost.to(torch.float32), dim=-1, descending=True, stable=True)
    slot, val = order.indices[..., :k], order.values[..., :k]
    off = offsets(r, cost.device)
    i = torch.arange(gh * gw, device=cost.device).view(1, -1, 1)
    qy, qx = torch.div(i, gw, rounding_mode="floor"), i % gw
    idx = (qy + off[:, 0][slot]) * gw + (qx + off[:, 1][slot])
    return idx.to(torch.int32), val.contiguous()


def soft_displacement(cost: torch.Tensor, radius: int, temperature: float = 0.1):
    """A sub-patch displacement field from a cost volume: cost [P, t, W * W] -> (flow [P, t, 2] fp32, conf [P, t] fp32).
    w = softmax(cost / temperature) over the slots in fp32 (the -inf slots outside the grid weigh 0), flow = sum over the
    slots, in slot order, of w * (dy, dx) -- in patches; multiply by the patch stride for pixels --, conf the largest weight
    (1: one candidate stands out; 1 / n: nothing does)."""
    r = check_local_radius("soft_displacement", radius)
    if _radius_of(cost, "soft_displacement") != r:
        raise ValueError(f"soft_displacement: cost has {cost.shape[2]} slots, radius {r} has {(2 * r + 1) ** 2}")
    if not float(temperature) > 0:
        raise ValueError(f"soft_displacement: temperature must be positive, got {temperature}")
    w = torch.softmax(cost.to(torch.float32) / float(temperature), dim=-1)
    off = offsets(r, cost.device).to(torch.float32)
    flow = w[..., 0, None] * off[0]
    for s in range(1, off.shape[0]):  # (the sum spelled out in slot order: torch's sum() fixes no order)
        flow = flow + w[..., s, None] * off[s]
    return flow, w.max(dim=-1).values


def vote_window(cost: torch.Tensor, src: torch.Tensor, grid, k: int, weights: str = "softmax", temperature: float = 0.1,
                labels: bool = True, neighbours: bool = True):
    """vdr.ops.window_vote in plain torch (CPU or device): the statement the kernel is read against, and what runs where there
    is no device.  cost [P, S, t, W * W] fp32, src [P, S, t, C] fp32 -> (scores [P, t, C] fp32, labels [P, t] int32, idx
    [P, t, k] int32 holding s * t + j, val [P, t, k] fp32), the op's arguments, refusals and definition (include/vdr.h):
    the slots outside the grid -- known from the grid, whatever they hold -- are no candidates; a stable descending sort of
    the concatenated [S * W * W] rows is the order (greater value, then lower source, then lower slot); e_m =
    exp((v_m - v_0) * (1 / T)) with 1 / T rounded once to fp32, or 1; both sums are spelled out in neighbour order from the
    first term, and there is one division per class.  Only the exponential may differ from the kernel's, by its error."""
    from .knn import lowest_argmax
    from .ops import check_window_vote
    P, S, gh, gw, r, k, C = check_window_vote("vote_window", cost, src, grid, k, weights, temperature)
    dev, t, WW = cost.device, gh * gw, (2 * r + 1) ** 2
    off = offsets(r, dev)
    i = torch.arange(t, device=dev).unsqueeze(1)
    cy, cx = torch.div(i, gw, rounding_mode="floor") + off[:, 0], i % gw + off[:, 1]  # [t, W * W]
    inside = (cy >= 0) & (cy < gh) & (cx >= 0) & (cx < gw)
    j = cy * gw + cx
    rows = torch.where(inside, cost, float("-inf")).permute(0, 2, 1, 3).reshape(P, t, S * WW)
    order = torch.sort(rows, dim=-1, descending=True, stable=True)
    e, val = order.indices[..., :k], order.values[..., :k].contiguous()
    s, w = torch.div(e, WW, rounding_mode="floor"), e % WW
    idx = s * t + torch.gather(j.unsqueeze(0).expand(P, t, WW), 2, w)  # [P, t, k]
    near = src.reshape(P, S * t, C)[torch.arange(P, device=dev).view(P, 1, 1), idx]  # [P, t, k, C]
    if weights == "uniform":
        em = torch.ones_like(val)
    else:
        inv_t = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(temperature), dtype=torch.float32))
        em = torch.exp((val - val[..., :1]) * inv_t)  # (a Python scalar that fp32 holds exactly: one fp32 multiplication)
    num, den = em[..., 0, None] * near[..., 0, :], em[..., 0]
    for m in range(1, k):  # (the sums spelled out in neighbour order: torch's sum() fixes no order)
        num = num + em[..., m, None] * near[..., m, :]
        den = den + em[..., m]
    scores = num / den.unsqueeze(-1)
    return (scores, lowest_argmax(scores).to(torch.int32) if labels else None, idx.to(torch.int32) if neighbours else None,
            val if neighbours else None)
