"""Batched slice pipeline around the encoder: the reference's per-slice hot loop
`generate_features` (src/tfds_dense_descriptor.py:242-284) with every slice of a volume in one batch, the ROI
maths of src/visualization_utils.py:93-125, and the HDF5 layout `save_features` (:142-165) writes, so
`train_models.py:147-157` reads the files unchanged.

Host-side integer logic (boxes, clamping) is restated here; pixels only move on the GPU (prep.prepare_slices ->
encoder -> vdr_op_crop_hwc) and come back once per volume, already cropped to the nodule box.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import prep


# ---- visualization_utils.py:93-125 ------------------------------------------------------------------------
def crop_box(shape_hw, xmin, ymin, xmax, ymax):
    """crop_image's clamping: the (y0, y1, x0, x1) slice bounds it applies to an array of spatial shape shape_hw."""
    h, w = shape_hw
    y0, y1 = [max(0, min(int(v), h)) for v in (ymin, ymax)]
    x0, x1 = [max(0, min(int(v), w)) for v in (xmin, xmax)]
    return y0, y1, x0, x1


def crop_image(img, xmin, ymin, xmax, ymax):
    y0, y1, x0, x1 = crop_box(img.shape[0:2], xmin, ymin, xmax, ymax)
    return img[y0:y1, x0:x1]


def extract_coords(mask, margin):
    """Box of a boolean mask; the reference's margins are asymmetric (ymin - m, xmin + m, ymax - m, xmax + m)."""
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        raise ValueError("empty mask")  # the reference raises here too (np.min of an empty array)
    ymin, xmin = int(ys.min()) - margin, int(xs.min()) + margin
    ymax, xmax = int(ys.max()) - margin, int(xs.max()) + margin
    h = max(ymax - ymin, margin)
    w = max(xmax - xmin, margin)
    return xmin, ymin, xmin + w, ymin + h


def roi_box(img_hw, mask, margin=1):
    """The box extract_roi crops an array of spatial shape img_hw to (rescaled when img and mask differ in size)."""
    xmin, ymin, xmax, ymax = extract_coords(mask, margin)
    mh, mw = mask.shape[0:2]
    if tuple(img_hw) != (mh, mw):
        h = img_hw[0] / mh
        w = img_hw[1] / mw
        xmin, ymin, xmax, ymax = [int(v) for v in (xmin * w, ymin * h, xmax * w, ymax * h)]
        hh = max(ymax - ymin, margin)
        ww = max(xmax - xmin, margin)
        xmax, ymax = xmin + ww, ymin + hh
    return xmin, ymin, xmax, ymax


def extract_roi(img, mask, margin=1):
    return crop_image(img, *roi_box(img.shape[0:2], mask, margin))


def crop_maps(maps: torch.Tensor, box) -> torch.Tensor:
    """maps fp32 [B, H, W, C] on the device -> [B, h', w', C] cropped to `box` = (xmin, ymin, xmax, ymax) with
    crop_image's clamping, by the HIP crop kernel."""
    lib = L.load()
    assert maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous() and maps.dim() == 4
    B, H, W, C = maps.shape
    y0, y1, x0, x1 = crop_box((H, W), *box)
    if y1 <= y0 or x1 <= x0:
        return torch.empty((B, max(y1 - y0, 0), max(x1 - x0, 0), C), dtype=torch.float32, device=maps.device)
    out = torch.empty((B, y1 - y0, x1 - x0, C), dtype=torch.float32, device=maps.device)
    L.check(lib.vdr_op_crop_hwc(maps.data_ptr(), out.data_ptr(), B, H, W, C, y0, x0, y1 - y0, x1 - x0,
                                torch.cuda.current_stream(maps.device).cuda_stream))
    return out


# ---- tfds_dense_descriptor.py:242-284 -----------------------------------------------------------------------
def generate_features(model, img_3d, mask_3d, flip=None, max_batch=16, descriptor=None):
    """Feature map of every slice, cropped to the nodule region.

    img_3d  (H, W, S) CT/PET volume in [0, 1] ('medsam') or (H, W, S, 3) ('dinov2'); mask_3d (H, W, S) bool.
    Returns (features_list, mask_list) exactly like the reference: per slice a (h', w', D) float32 array and
    the (h'', w'') bool mask crop.  All S slices go through prepare -> encoder -> ROI crop in batches of
    `max_batch` on the GPU; one D2H per batch of the already-cropped maps.

    flip ('horizontal' | 'vertical' | None): the result is that of the reference's
    `generate_features(model, *flip_image(img_3d, mask_3d, flip))` (tfds_dense_descriptor.py:463-467): the mask is
    flipped first, every box (volume crop, ROI of the feature maps, ROI of the masks -- asymmetric margins and all) is
    derived from the FLIPPED mask, and the pixels are read from the mirrored window of the unflipped volume with the
    reversal folded into the resize gather (no flipped copy of the volume is made).

    descriptor (None: the reference's maps, as above): a dict of VitDescriptorModel.extract_descriptors' keywords --
    layer, facet, bin, hierarchy -- for facet descriptors instead (ViT / DINOv2 / CLIP models): the per-slice maps are
    (h', w', d) with d = D, or (1 + 8*hierarchy)*D with bin=True; the ROI crop works on that channel count.
    descriptor["upsample"] (a dict of radius, sigma_spatial, sigma_range; {} for the defaults): the descriptors come at PIXEL
    resolution by guided upsampling (VitDescriptorModel.upsample_descriptors, guided by the prepared slice itself).  The ROI
    box of the feature maps is then taken in pixel coordinates of the prepared slice and only that box is upsampled; the mask
    crops are taken from the mask resampled (nearest) to the prepared slice under the same box, so the feature crops and the
    mask crops have the same height and width.  Without the key the function is what it was."""
    desc = up = None
    if descriptor is not None:
        unknown = set(descriptor) - {"layer", "facet", "bin", "hierarchy", "upsample"}
        if unknown:
            raise ValueError(f"descriptor: unknown keys {sorted(unknown)} (layer, facet, bin, hierarchy, upsample)")
        if descriptor.get("upsample") is not None:
            up = dict(descriptor["upsample"])
            unknown = set(up) - {"radius", "sigma_spatial", "sigma_range"}
            if unknown:
                raise ValueError(f"descriptor['upsample']: unknown keys {sorted(unknown)} (radius, sigma_spatial, sigma_range)")
            from . import ops
            if not 1 <= int(up.get("radius", 2)) <= ops.UPSAMPLE_MAX_RADIUS:
                raise ValueError(f"descriptor['upsample']: radius must be 1..{ops.UPSAMPLE_MAX_RADIUS}, got {up['radius']}")
            ops.upsample_coefficients(1, up.get("sigma_spatial", 1.0), up.get("sigma_range", 0.1))
        desc = {"layer": descriptor.get("layer"), "facet": descriptor.get("facet", "key"), "bin": bool(descriptor.get("bin", False)),
                "hierarchy": int(descriptor.get("hierarchy", 2))}
        model._descriptor_args(desc["layer"], desc["facet"], desc["bin"], False, desc["hierarchy"])  # (before any device work)
    if flip not in (None, "horizontal", "vertical"):
        raise ValueError(f"flip must be None, 'horizontal' or 'vertical', got {flip!r}")
    mask_np = mask_3d.cpu().numpy() if isinstance(mask_3d, torch.Tensor) else np.asarray(mask_3d)
    if flip == "horizontal":
        mask_np = mask_np[:, ::-1]
    elif flip == "vertical":
        mask_np = mask_np[::-1]
    bigger_mask = np.sum(mask_np, axis=-1) > 0
    xmin, ymin, xmax, ymax = extract_coords(bigger_mask, margin=2)
    crop_size = max(xmax - xmin, ymax - ymin) * 2
    xmid, ymid = int(xmin + (xmax - xmin) / 2), int(ymin + (ymax - ymin) / 2)
    box = (xmid - crop_size, ymid - crop_size, xmid + crop_size, ymid + crop_size)

    vol = torch.as_tensor(img_3d)
    y0, y1, x0, x1 = crop_box(vol.shape[0:2], *box)   # in the coordinates of the flipped volume
    vy0, vy1, vx0, vx1 = y0, y1, x0, x1              # the same window in the unflipped volume: mirrored
    if flip == "horizontal":
        vx0, vx1 = vol.shape[1] - x1, vol.shape[1] - x0
    elif flip == "vertical":
        vy0, vy1 = vol.shape[0] - y1, vol.shape[0] - y0
    vol = vol[vy0:vy1, vx0:vx1]                  # a view; prepare_slices reads it strided (and reversed, for a flip)
    mask_c = mask_np[y0:y1, x0:x1]
    bigger_c = bigger_mask[y0:y1, x0:x1]
    vol = vol.to(model.device)
    if vol.dtype not in (torch.float32, torch.float64):
        vol = vol.to(torch.float32)
    S = vol.shape[2]
    features_list, mask_list = [], []
    rb = mb = None
    pending = []
    for s0 in range(0, S, max_batch):
        s1 = min(S, s0 + max_batch)
        # bf16 pixels: the patch GEMM rounds them to bf16 in any case (same round-to-nearest-even, same features bit
        # for bit); written as bf16 here they are half the bytes, and for p = 16 (MedSAM) the GEMM gathers them straight
        # from the images (no im2col pass)
        x = prep.prepare_slices(vol[:, :, s0:s1], side=model.cfg.img, flip=flip, out_dtype=torch.bfloat16, device=model.device)
        if up is not None:
            if rb is None:  # (pixel coordinates of the prepared slice; the masks resampled to it, nearest)
                side_hw = tuple(int(v) for v in x.shape[-2:])
                rb = mb = roi_box(side_hw, bigger_c)
                ry = (np.arange(side_hw[0]) * mask_c.shape[0]) // side_hw[0]
                rx = (np.arange(side_hw[1]) * mask_c.shape[1]) // side_hw[1]
                mask_c = mask_c[ry][:, rx]
            by0, by1, bx0, bx1 = crop_box(x.shape[-2:], *rb)
            if by1 <= by0 or bx1 <= bx0:
                raise ValueError(f"generate_features: the ROI box {rb} lies outside the prepared slice")
            crops = model.upsample_descriptors(x, box=(by0, bx0, by1, bx1), out_dtype=torch.float32, **desc, **up)
            host = torch.empty(crops.shape, dtype=crops.dtype, pin_memory=True)
            host.copy_(crops, non_blocking=True)
            pending.append((host, s0, s1))
            continue
        if desc is not None:
            maps = model.extract_descriptors(x, reshape=True, **desc)             # [b, gh, gw, d] channel-last
        else:  # the model's own: a SAM encoder's neck output [b, g, g, C], else patch_embed on the grid in force
            maps = model._dense_map(x)
        if rb is None:  # the boxes depend on the (cropped) union mask only: once per volume, not once per slice
            rb = roi_box(maps.shape[1:3], bigger_c)
            mb = roi_box(mask_c.shape[0:2], bigger_c)
        crops = crop_maps(maps.contiguous(), rb)
        host = torch.empty(crops.shape, dtype=crops.dtype, pin_memory=True)
        host.copy_(crops, non_blocking=True)   # D2H queued behind the crop; the next batch is enqueued without a host sync
        pending.append((host, s0, s1))
    torch.cuda.current_stream(model.device).synchronize()  # ONE synchronisation per volume
    for host, s0, s1 in pending:
        arr = host.numpy()
        for i in range(s1 - s0):
            features_list.append(arr[i])
            mask_list.append(crop_image(mask_c[:, :, s0 + i] > 0, *mb))
    return features_list, mask_list


def _check_regions(what, min_region_area, fill_holes, keep_largest):
    """The region keywords of segment_volume / propagate_segmentation -> whether any is on; ValueError before any device work"""
    if isinstance(min_region_area, bool) or not isinstance(min_region_area, int) or min_region_area < 0:
        raise ValueError(f"{what}: min_region_area must be an integer >= 0, got {min_region_area!r}")
    if not isinstance(fill_holes, bool) or not isinstance(keep_largest, bool):
        raise ValueError(f"{what}: fill_holes and keep_largest must be True or False, got {fill_holes!r}, {keep_largest!r}")
    if fill_holes and min_region_area == 0:
        raise ValueError(f"{what}: fill_holes fills the holes below min_region_area pixels: give a positive min_region_area")
    return min_region_area > 0 or keep_largest


def _region_kwargs(min_region_area, fill_holes, keep_largest):
    """the clean() keywords: holes below the area filled when asked; islands below it removed, or only the largest part kept"""
    return dict(min_area=min_region_area, holes=fill_holes, islands=min_region_area > 0 and not keep_largest, largest=keep_largest)


def _check_grow(what, grow, spatial_res):
    """the checks of grow / spatial_res before any device work -> the spacing (sz, sy, sx) of the [S, H, W] mask volume, or None.
    spatial_res is in the reference's (x, y, z) order, as tfds2voxels returns it."""
    from . import morphology as mo
    if spatial_res is None:
        mo.check_radius(what + ": grow", grow)
        return None
    try:
        res = tuple(float(v) for v in spatial_res)
    except (TypeError, ValueError):
        res = ()
    if len(res) != 3:
        raise ValueError(f"{what}: spatial_res must be the voxel size (x, y, z), got {spatial_res!r}")
    spacing = (res[2], res[1], res[0])
    try:
        _, quantum = mo.quantize_spacing(spacing)
    except ValueError as e:
        raise ValueError(f"{what}: spatial_res: {e}") from None
    mo.radius_squared(what + ": grow", grow, quantum)
    return spacing


def _grow(what, masks, grow, spacing=None):
    """Euclidean dilation of finished bool masks [S, H, W] on the device by `grow` (vdr.morphology.dilate): slice by slice by the
    disc of that many pixels, or, with the spacing (sz, sy, sx) of the volume, by the 3-D ellipsoid of that length; 0: the masks"""
    from . import morphology as mo
    if spacing is not None:
        return mo.dilate(masks, grow, spacing=spacing)
    return masks if mo.check_radius(what, grow) == 0 else mo.dilate(masks, grow)


def segment_volume(model, img_3d, boxes, max_batch=16, threshold=0.0, min_region_area=0, fill_holes=False, keep_largest=False, grow=0.0, spatial_res=None):
    """The mask generate_features takes as mask_3d, from box prompts: img_3d (H, W, S) gray volume in [0, 1] (or (H, W, S, 3)),
    boxes [S, 4] (x0, y0, x1, y1) in slice pixels, one per slice, or one box [4] for every slice -> (H, W, S) bool numpy.
    The slices run in chunks of `max_batch` through prepare -> model.segment (mask token 0) -> bilinear logits at slice
    resolution > threshold; one synchronisation per volume.  SAM / MedSAM models loaded with their decoder weights.
    min_region_area > 0 removes, slice by slice, the islands below that many pixels (the largest stays when all are), fill_holes
    also fills the holes below it, keep_largest keeps only each slice's largest component (Segmentation.clean: connected
    components on the device, 8-connected, 2-D).  All three off is the path without them, bit for bit.  grow > 0 dilates the
    finished mask of every slice, after any cleaning, by the Euclidean disc of that radius in slice pixels (compared as
    floor(grow^2); one distance transform on the device); 0 is the path without it.  spatial_res = the voxel size (x, y, z) as
    tfds2voxels returns it: grow is then a LENGTH in that unit and the dilation is the 3-D ellipsoid over the finished volume
    (vdr.morphology.dilate with spacing: one thresholded 3-D transform, the spacing rounded to 2^-10 of its unit); None is the
    slice-by-slice path, bit for bit."""
    from . import segment as sg
    regions = _check_regions("segment_volume", min_region_area, fill_holes, keep_largest)
    spacing = _check_grow("segment_volume", grow, spatial_res)
    sg._require(model, "segment_volume")
    vol = torch.as_tensor(img_3d)
    if vol.dim() not in (3, 4) or (vol.dim() == 4 and vol.shape[3] != 3):
        raise ValueError(f"segment_volume: img_3d must be (H, W, S) or (H, W, S, 3), got {tuple(vol.shape)}")
    H, W, S = (int(v) for v in vol.shape[:3])
    b = torch.as_tensor(boxes)
    if tuple(b.shape) not in ((4,), (S, 4)):
        raise ValueError(f"segment_volume: boxes must be [4] or [{S}, 4], got {tuple(b.shape)}")
    sg.check_boxes("segment_volume", b.reshape(-1, 1, 4))
    b = b.double().reshape(-1, 4).expand(S, 4)
    side = model.cfg.img
    scaled = b * torch.tensor([side / W, side / H, side / W, side / H], dtype=torch.float64)   # (segment.scale_box, per slice)
    vol = vol.to(model.device)
    if vol.dtype not in (torch.float32, torch.float64):
        vol = vol.to(torch.float32)
    out = torch.empty((S, H, W), dtype=torch.bool, device=model.device)
    for s0 in range(0, S, max_batch):
        s1 = min(S, s0 + max_batch)
        x = prep.prepare_slices(vol[:, :, s0:s1], side=side, device=model.device)
        seg = model.segment(x, scaled[s0:s1].reshape(s1 - s0, 1, 4))
        if regions:
            out[s0:s1] = seg.clean(size=(H, W), threshold=threshold, **_region_kwargs(min_region_area, fill_holes, keep_largest))[0][:, 0, 0]
        else:
            out[s0:s1] = seg.masks(size=(H, W), threshold=threshold)[:, 0, 0]
    return _grow("segment_volume: grow", out, grow, spacing).permute(1, 2, 0).cpu().numpy()


def propagate_segmentation(model, img_3d, box, index, direction="both", margin=8, use_mask_prompt=True, max_batch=16, threshold=0.0,
                           min_region_area=0, fill_holes=False, keep_largest=False, grow=0.0, point_prompt=None, spatial_res=None):
    """segment_volume from ONE annotation: img_3d (H, W, S) gray volume in [0, 1] (or (H, W, S, 3)), box (x0, y0, x1, y1) in
    slice pixels on slice `index` -> (H, W, S) bool numpy, the array generate_features takes as mask_3d.  The slices are
    prepared in chunks of max_batch, model.propagate_masks carries the mask through the volume (margin in pixels of the
    prepared input), the logits are resampled to slice resolution; one synchronisation per volume.  min_region_area, fill_holes and
    keep_largest as segment_volume's: they clean the RETURNED masks slice by slice, the propagation itself is untouched; grow as
    segment_volume's, after the cleaning.  point_prompt: model.propagate_masks' (None, or "inner" for the neighbour's most
    interior pixel as a positive click on every further slice).  spatial_res: segment_volume's (grow as a length, the 3-D
    ellipsoid over the finished volume); None is the slice-by-slice path, bit for bit."""
    from . import segment as sg
    regions = _check_regions("propagate_segmentation", min_region_area, fill_holes, keep_largest)
    spacing = _check_grow("propagate_segmentation", grow, spatial_res)
    if point_prompt not in (None, "inner"):
        raise ValueError(f"propagate_segmentation: point_prompt must be None or 'inner', got {point_prompt!r}")
    sg._require(model, "propagate_segmentation")
    vol = torch.as_tensor(img_3d)
    if vol.dim() not in (3, 4) or (vol.dim() == 4 and vol.shape[3] != 3):
        raise ValueError(f"propagate_segmentation: img_3d must be (H, W, S) or (H, W, S, 3), got {tuple(vol.shape)}")
    H, W, S = (int(v) for v in vol.shape[:3])
    b = torch.as_tensor(box)
    if tuple(b.shape) != (4,):
        raise ValueError(f"propagate_segmentation: box must be (x0, y0, x1, y1), got {tuple(b.shape)}")
    sg.check_boxes("propagate_segmentation", b.reshape(1, 1, 4))
    if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < S:
        raise ValueError(f"propagate_segmentation: index must be a slice number in [0, {S}), got {index!r}")
    side = model.cfg.img
    scaled = torch.tensor(sg.scale_box(b.tolist(), H, W, side), dtype=torch.float64)
    vol = vol.to(model.device)
    if vol.dtype not in (torch.float32, torch.float64):
        vol = vol.to(torch.float32)
    x = torch.cat([prep.prepare_slices(vol[:, :, s0:s0 + max_batch], side=side, device=model.device) for s0 in range(0, S, max_batch)], dim=0)
    kw = {} if point_prompt is None else dict(point_prompt=point_prompt)
    seg = model.propagate_masks(x, scaled, index, direction=direction, margin=margin, use_mask_prompt=use_mask_prompt, max_batch=max_batch, **kw)
    if regions:
        masks = seg.clean(size=(H, W), threshold=threshold, **_region_kwargs(min_region_area, fill_holes, keep_largest))[0]
    else:
        masks = seg.masks(size=(H, W), threshold=threshold)
    return _grow("propagate_segmentation: grow", masks, grow, spacing).permute(1, 2, 0).cpu().numpy()


# ---- tfds_dense_descriptor.py:142-165 -----------------------------------------------------------------------
from .h5store import read_features, save_features  # noqa: E402,F401  (torch-free module: also runs where only h5py is)


# ---- tfds_dense_descriptor.py:452-491 ------------------------------------------------------------------------
AUGMENTATIONS = [(flip, angle) for flip in (None, "horizontal", "vertical") for angle in range(0, 180, 45)]


def feature_metadata(n_features_per_aug, patient_id, label, dataset_name, modality, spatial_res, augmentations=None):
    """The per-patient table the reference stores next to the HDF5 features (`{patient}_{modality}.parquet`):
    one row per feature map, columns feature_id, slice, angle, flip, patient_id, label, dataset, modality,
    augmentation, spatial_res — what train_models.py:147-157 / prepare_df read.

    n_features_per_aug: number of slices produced for each (flip, angle) in `augmentations` (default: the
    reference's 3 flips x 4 angles, in its loop order).  `augmentation` is True on every row: the reference
    computes `not (df['flip'] is None and angle == 0)` with `df['flip'] is None` evaluated on the Series object
    (always False), and consumers were written against that output."""
    import pandas as pd

    augmentations = AUGMENTATIONS if augmentations is None else list(augmentations)
    if isinstance(n_features_per_aug, int):
        n_features_per_aug = [n_features_per_aug] * len(augmentations)
    rows = {"slice": [], "angle": [], "flip": []}
    for (flip, angle), n in zip(augmentations, n_features_per_aug):
        rows["angle"] += [angle] * n
        rows["flip"] += [flip] * n
        rows["slice"] += list(range(n))
    df = pd.DataFrame(rows)
    df.reset_index(drop=False, inplace=True)
    df = df.rename(columns={"index": "feature_id"})
    df["patient_id"] = patient_id
    df["label"] = label
    df["dataset"] = dataset_name.replace("_dataset", "")
    df["modality"] = modality
    df["augmentation"] = True
    df["spatial_res"] = [spatial_res] * df.shape[0]
    return df


def rotate_image(image, mask, angle, axes=(0, 1)):
    """tfds_dense_descriptor.py:327-350 on the GPU (prep.rotate_image: SciPy's cubic-spline rotation restated in
    float64, bit-identical): image clipped to [0, 1], mask > 0.  numpy in -> numpy out (the reference's contract);
    device tensors in -> device tensors out, which generate_features consumes without another upload."""
    on_host = not (isinstance(image, torch.Tensor) and image.is_cuda)
    img, m = prep.rotate_image(image, mask, angle, axes=axes)
    if on_host:
        return img.cpu().numpy(), m.cpu().numpy()
    return img, m


def extract_patient_features(model, img_raw, mask_raw, patient_id, label, dataset_name, modality, spatial_res,
                             flips=(None, "horizontal", "vertical"), angles=(0, 45, 90, 135), max_batch=16):
    """The reference's per-patient augmentation loop (tfds_dense_descriptor.py:452-491): for every flip x angle,
    generate_features over the whole volume; returns (all_features, all_masks, metadata DataFrame) ready for
    save_features / save_metadata.  The volume and its mask are uploaded ONCE; flips (torch.flip), rotations
    (prep.rotate_image), resize, encoder and ROI crop all run on the GPU, and only the cropped feature maps and the
    rotated masks (needed for the boxes) come back."""
    all_features, all_masks, counts, augs = [], [], [], []
    img = torch.as_tensor(np.asarray(img_raw) if not isinstance(img_raw, torch.Tensor) else img_raw)
    if img.dtype not in (torch.float32, torch.float64):
        # scipy.ndimage.rotate on an INTEGER volume rounds its result back to the integer dtype; that store is not
        # restated on the GPU (prep.rotate_volume refuses integers), and the reference's volumes are floats at this
        # point (apply_window_ct / PET SUV): refuse rather than rotate something SciPy would round differently
        if any(a != 0 for a in angles):
            raise TypeError(f"extract_patient_features rotates float32 / float64 volumes only, got {img.dtype}; "
                            "convert explicitly (the reference passes windowed CT / PET floats)")
        img = img.to(torch.float64)
    img = img.to(model.device)
    mask = torch.as_tensor(np.asarray(mask_raw) if not isinstance(mask_raw, torch.Tensor) else mask_raw).to(model.device)
    mask = mask if mask.dtype == torch.bool else mask > 0

    for flip_type in flips:
        im_f, m_f = prep.flip_image(img, mask, flip_type)  # flip_image (:305-324)
        for angle in angles:
            im, m = (im_f, m_f) if angle == 0 else prep.rotate_image(im_f, m_f, angle)
            feats, fmasks = generate_features(model, im, m, max_batch=max_batch)
            all_features += feats
            all_masks += fmasks
            counts.append(len(feats))
            augs.append((flip_type, angle))
    df = feature_metadata(counts, patient_id, label, dataset_name, modality, spatial_res, augmentations=augs)
    return all_features, all_masks, df


def save_metadata(df, df_path):
    df.to_parquet(df_path)


# ---- train_models.py:30-44, :143-182 --------------------------------------------------------------------------
def resize_mask_nearest(mask, out_hw):
    """skimage.transform.resize(mask, out_hw, order=0) of a boolean mask (nearest sample of the pixel-centre
    mapping, = scipy.ndimage.zoom(order=0, grid_mode=True), what current skimage calls)."""
    mask = np.asarray(mask)
    H, W = mask.shape
    oh, ow = out_hw
    yi = np.clip(np.floor((np.arange(oh) + 0.5) * H / oh - 0.5 + 0.5).astype(np.int64), 0, H - 1)
    xi = np.clip(np.floor((np.arange(ow) + 0.5) * W / ow - 0.5 + 0.5).astype(np.int64), 0, W - 1)
    return mask[yi][:, xi].astype(bool)


def masked_voxel_sequence(slice_features, slice_masks, spatial_res, noise=(0.0, 0.0, 0.0), out_dtype=torch.float32,
                          device=None):
    """The Stage-C input of one patient and modality, as the 'transformer' branch of PETCTDataset3D._get_features
    builds it (train_models.py:143-182): per-slice (h, w, D) feature maps + nodule masks -> [n, D] sequence of the
    masked voxels, each with its 3-D sinusoidal position code / 4 added (positional_encoding_3d, :30-44).

    Host side (integer / small float64 logic, restated): nearest mask resize, kept-voxel indices, coordinates — with
    the reference's np.meshgrid 'xy' flat order, mean-centring and `noise` offsets.  Device side
    (vdr_op_voxel_sequence): gather + sin / cos + add, float64 like numpy, rounded once to `out_dtype`.
    slice_features may be numpy arrays (uploaded once) or one device tensor [S, h, w, D]."""
    lib = L.load()
    if isinstance(slice_features, torch.Tensor):
        feats = slice_features
    else:
        feats = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) for f in slice_features], axis=0))
    dev = device if device is not None else (feats.device if feats.is_cuda else "cuda")
    S, h, w, D = feats.shape
    vol = feats.to(dev, torch.float32).permute(1, 2, 0, 3).contiguous().view(-1, D)       # (h, w, S) positions
    masks = np.stack([resize_mask_nearest(m, (h, w)) for m in slice_masks], axis=0)
    keep = np.transpose(masks, (1, 2, 0)).reshape(-1)
    h0, w0 = np.asarray(slice_masks[-1]).shape[0:2]
    x, y, z = np.meshgrid(np.arange(0, h), np.arange(0, w), np.arange(0, S))              # 'xy' indexing, as the reference
    x = (x.flatten() / w).flatten() * w0 * spatial_res[0]
    y = (y.flatten() / h).flatten() * h0 * spatial_res[1]
    z = (z.flatten()).flatten() * spatial_res[2]
    xyz = np.stack([(x - x.mean() + noise[0])[keep], (y - y.mean() + noise[1])[keep], (z - z.mean() + noise[2])[keep]])
    index = np.flatnonzero(keep).astype(np.int64)
    n = int(index.shape[0])
    out = torch.empty((n, D), dtype=out_dtype, device=vol.device)
    if n == 0:
        return out
    expo = np.array([10000 ** (6 * i / D) for i in range(D // 6)], dtype=np.float64)
    d_index = torch.from_numpy(index).to(vol.device)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64)).to(vol.device)
    d_expo = torch.from_numpy(expo).to(vol.device)
    odt = {torch.float32: L.VDR_F32, torch.bfloat16: L.VDR_BF16, torch.float64: L.VDR_F64}[out_dtype]
    L.check(lib.vdr_op_voxel_sequence(vol.data_ptr(), d_index.data_ptr(), d_xyz.data_ptr(), d_expo.data_ptr(), n, D,
                                      out.data_ptr(), odt, torch.cuda.current_stream(vol.device).cuda_stream))
    return out
