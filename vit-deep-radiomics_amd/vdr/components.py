"""Connected components of mask planes (include/vdr.h "connected components"; the kernels are csrc/components.hip and are reached
through vdr.ops.connected_components / mask_clean / mask_binarize).

A plane is [H, W], nonzero = set, pixel index i = y * W + x.  The ROOT of a selected pixel is the lowest pixel index of its
component, -1 for a pixel that is not selected; the AREA of a component is its pixel count, stored at the root.  Both are
functions of the partition alone, so they can be held bit for bit to any other labelling (scipy.ndimage.label: `relabel` gives
its numbering).

label_torch and clean_torch state the two ops in plain torch on the CPU: the kernels are read against them bit for bit.
relabel, seed_component and largest are small pure-torch helpers on a root plane; they run on whatever device the planes are on
and do not synchronise.

Deviations: components are 2-D, plane by plane (a volume is cleaned slice-wise); "largest" ties go to the lowest root; parity
with OpenCV's connectedComponentsWithStats is unpinned (its numbering agrees by construction, its tie order for the largest
component is not known)."""
from __future__ import annotations

import torch

HOLES, ISLANDS, LARGEST = 1, 2, 4   # VDR_CLEAN_* (include/vdr.h)
MAX_SIDE = 4096                     # VDR_COMPONENTS_MAX_SIDE


def as_planes(mask, what: str):
    """A bool / uint8 mask of 2 or 3 dimensions -> ([P, H, W] uint8 contiguous, whether a plane dimension was added)"""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() not in (2, 3):
        raise ValueError(f"{what}: mask must be a bool or uint8 tensor [H, W] or [P, H, W]")
    single = mask.dim() == 2
    m = mask[None] if single else mask
    P, H, W = (int(v) for v in m.shape)
    if not (1 <= P <= 65535 and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: 1 .. 65535 planes with sides of 1 .. {MAX_SIDE}, got {tuple(mask.shape)}")
    m = m.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), single


def as_volumes(vol, what: str):
    """A bool / uint8 mask of 3 or 4 dimensions, the last three one volume -> ([P, Z, H, W] uint8 contiguous, whether a volume
    dimension was added).  The P Z slices go through as_planes, the one operand check of the mask-plane ops; a volume has at most
    2^30 voxels."""
    if not isinstance(vol, torch.Tensor) or vol.dtype not in (torch.bool, torch.uint8) or vol.dim() not in (3, 4):
        raise ValueError(f"{what}: mask must be a bool or uint8 tensor [Z, H, W] or [P, Z, H, W]")
    single = vol.dim() == 3
    v = vol[None] if single else vol
    P, Z, H, W = (int(n) for n in v.shape)
    if not (P >= 1 and 1 <= Z <= MAX_SIDE and Z * H * W <= 2**30):
        raise ValueError(f"{what}: volumes of 1 .. {MAX_SIDE} slices and at most 2^30 voxels, got {tuple(vol.shape)}")
    planes, _ = as_planes(v.reshape(P * Z, H, W), what)
    return planes.reshape(P, Z, H, W), single


def check_connectivity(what: str, connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def check_clean(what: str, min_area, holes, islands, largest, connectivity) -> "tuple[int, int, int]":
    """(min_area, mode, connectivity) of a clean call, or ValueError"""
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 0 or min_area > 2**31 - 1:
        raise ValueError(f"{what}: min_area must be an integer >= 0, got {min_area!r}")
    if islands and largest:
        raise ValueError(f"{what}: islands and largest exclude each other")
    return int(min_area), (HOLES if holes else 0) | (ISLANDS if islands else 0) | (LARGEST if largest else 0), check_connectivity(what, connectivity)


# ---- the torch statements -------------------------------------------------------------------------------------------------------
def label_torch(mask: torch.Tensor, connectivity: int = 8, value: int = 1, device="cpu"):
    """vdr_op_connected_components in torch, on the CPU unless told otherwise: masked minimum propagation to a fixed point.  mask
    [P, H, W] or [H, W] -> (root int32, area int32, count int32 [P]).  Every selected pixel starts with its own index and takes
    the minimum over its selected neighbours until nothing changes: the fixed point is the lowest index of the component.
    (device: the same statement on another device, as a yardstick; every round ends in one synchronisation.)"""
    m, single = as_planes(mask.detach().to(device), "label_torch")
    check_connectivity("label_torch", connectivity)
    P, H, W = m.shape
    dev = m.device
    sel = (m != 0) == bool(value)
    big = H * W
    lab = torch.where(sel, torch.arange(H * W, dtype=torch.int64, device=dev).reshape(1, H, W).expand(P, H, W), torch.full((), big, dtype=torch.int64, device=dev))
    shifts = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    while True:
        pad = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=big)
        new = lab
        for dy, dx in shifts:
            new = torch.minimum(new, pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        new = torch.where(sel, new, lab)
        # pointer jumping: a label is a pixel of the same component, so that pixel's label is one too and is no larger; it only
        # shortens the way to the same fixed point (a one-pixel-wide path of length n would otherwise take n rounds)
        table = torch.cat([new.reshape(P, -1), torch.full((P, 1), big, dtype=torch.int64, device=dev)], dim=1)
        new = torch.gather(table, 1, new.reshape(P, -1)).reshape(P, H, W)
        if bool((new == lab).all()):
            break
        lab = new
    root = torch.where(sel, lab, torch.full((), -1, dtype=torch.int64, device=dev))
    area = torch.zeros((P, H * W + 1), dtype=torch.int64, device=dev)
    area.scatter_add_(1, lab.reshape(P, -1), sel.reshape(P, -1).to(torch.int64))   # unselected pixels add 0 to the spare slot
    area = area[:, :H * W].reshape(P, H, W)
    count = (area > 0).reshape(P, -1).sum(dim=1)
    root, area, count = root.to(torch.int32), area.to(torch.int32), count.to(torch.int32)
    return (root[0], area[0], count) if single else (root, area, count)


def _stats(out: torch.Tensor) -> torch.Tensor:
    P = out.shape[0]
    stats = torch.zeros((P, 5), dtype=torch.int32)
    for p in range(P):
        m = out[p] != 0
        if bool(m.any()):
            ys, xs = m.any(dim=1).nonzero()[:, 0], m.any(dim=0).nonzero()[:, 0]
            stats[p] = torch.stack([m.sum(), xs[0], ys[0], xs[-1], ys[-1]]).to(torch.int32)
    return stats


def clean_torch(mask: torch.Tensor, min_area: int = 0, holes: bool = False, islands: bool = False, largest: bool = False, connectivity: int = 8):
    """vdr_op_mask_clean in torch on the CPU -> (out uint8, changed int32 [P], stats int32 [P, 5]); the steps in the header's
    order, each on the result of the one before"""
    m, single = as_planes(mask.detach().cpu(), "clean_torch")
    min_area, mode, connectivity = check_clean("clean_torch", min_area, holes, islands, largest, connectivity)
    P, H, W = m.shape
    cur = (m != 0)
    changed = torch.zeros(P, dtype=torch.int32)

    def area_of(root, area):   # the area of every selected pixel's component (0 where not selected)
        return torch.gather(area.reshape(P, -1).to(torch.int64), 1, root.reshape(P, -1).clamp_min(0).to(torch.int64)).reshape(P, H, W) * (root >= 0)
    if mode & HOLES:
        root, area, _ = label_torch(cur, connectivity, 0)
        fill = (root >= 0) & (area_of(root, area) < min_area)
        changed |= fill.reshape(P, -1).any(dim=1).to(torch.int32)
        cur = cur | fill
    if mode & (ISLANDS | LARGEST):
        root, area, _ = label_torch(cur, connectivity, 1)
        best = largest_root(area)
        is_best = root == best[:, None, None]
        keep = is_best if mode & LARGEST else (area_of(root, area) >= min_area) | is_best
        new = cur & keep
        changed |= 2 * (new != cur).reshape(P, -1).any(dim=1).to(torch.int32)
        cur = new
    out = cur.to(torch.uint8)
    stats = _stats(out)
    return (out[0], changed, stats) if single else (out, changed, stats)


# ---- helpers on a root plane: pure torch, any device, no synchronisation ---------------------------------------------------------
def relabel(root: torch.Tensor) -> torch.Tensor:
    """root int32 [.., H, W] -> labels int32: 0 for background, then 1, 2, .. in the order of the components' first pixels
    (scipy.ndimage.label's numbering): the running count of root pixels, gathered by root"""
    H, W = root.shape[-2:]
    flat = root.reshape(-1, H * W).to(torch.int64)
    is_root = flat == torch.arange(H * W, device=root.device)
    rank = torch.cumsum(is_root.to(torch.int64), dim=1)
    lab = torch.gather(rank, 1, flat.clamp_min(0)) * (flat >= 0)
    return lab.to(torch.int32).reshape(root.shape)


def seed_component(root: torch.Tensor, seed: torch.Tensor) -> torch.Tensor:
    """root int32 [P, H, W], seed int64 [P] flat pixel indices -> bool [P, H, W]: the component that holds the seed (nothing when
    the seed is not selected)"""
    P, H, W = root.shape
    r = torch.gather(root.reshape(P, -1), 1, seed.reshape(P, 1).to(torch.int64))
    return (root == r[:, :, None]) & (r[:, :, None] >= 0)


def largest_root(area: torch.Tensor) -> torch.Tensor:
    """area int32 [P, H, W] -> int64 [P]: the root of the largest component, the lowest on a tie; -1 for a plane without one"""
    P = area.shape[0]
    flat = area.reshape(P, -1).to(torch.int64)
    n = flat.shape[1]
    key = flat * n + (n - 1 - torch.arange(n, device=area.device))   # the larger area first, then the lower index
    best = key.argmax(dim=1)
    return torch.where(flat.gather(1, best[:, None])[:, 0] > 0, best, torch.full_like(best, -1))


def largest(root: torch.Tensor, area: torch.Tensor) -> torch.Tensor:
    """bool [P, H, W]: the largest component of every plane (ties: the lowest root)"""
    return (root == largest_root(area)[:, None, None].to(root.dtype)) & (root >= 0)
