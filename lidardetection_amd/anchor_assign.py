"""Host side of csrc/anchor_assign.hip: anchor target assignment (AxisAlignedTargetAssigner on its deterministic path,
pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py) for a whole batch and every anchor class in one call.

The class tables (gt class id -> anchor class, thresholds, output layout) are built once on the host; a call allocates the
outputs and a workspace from torch's caching allocator, launches on the current stream and never synchronises."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 16      # anchor classes per call (csrc/anchor_assign.hip: AA_MAX_CLASSES)
ID_MIN, NUM_IDS = -64, 128   # gt class ids -64..63 have a table entry (AA_ID_MIN, AA_NUM_IDS)
MAX_CODE = 16         # code_size (AA_MAX_CODE)


def class_table(class_names, anchor_class_names):
    """anchor class index (or -1) of the gt class ids -64..63, in that order (entry id - ID_MIN).  The reference masks a gt of id c
    into the anchor class named class_names[c - 1] (axis_aligned_target_assigner.py:61-66) with numpy indexing: id 0 wraps to the
    LAST class name and negative ids wrap further, as here.  Ids whose name has no anchor class match none; so do ids past the
    name list, where the reference raises IndexError (the device cannot raise without a host synchronisation)."""
    names = list(class_names)
    if len(set(anchor_class_names)) != len(anchor_class_names):
        raise ValueError(f"anchor class names must be unique, got {list(anchor_class_names)}")
    table = []
    for cid in range(ID_MIN, ID_MIN + NUM_IDS):
        j = cid - 1
        name = names[j] if -len(names) <= j < len(names) else None
        table.append(list(anchor_class_names).index(name) if name in anchor_class_names else -1)
    return table


def output_layout(anchor_shapes, use_multihead):
    """anchor_shapes: per-class [z, y, x, size, rot, ndim] shapes (AnchorGenerator) -> (per_loc, out_off, a_total).
    Anchor i of class k goes to output anchor (i // per_loc[k]) * a_total + out_off[k] + i % per_loc[k]:
      single head: the per-class targets are view(*feature_map_size, -1) and concatenated on the last axis (:102-115), so a
                   location holds every class's R_k anchors in class order;
      multihead:   the anchors were permuted (3, 4, 0, 1, 2, 5) and the per-class targets are concatenated (:92-100)."""
    counts = [int(np.prod(s[:-1])) for s in anchor_shapes]
    if use_multihead:
        out_off = [int(x) for x in np.cumsum([0] + counts[:-1])]
        return [max(n, 1) for n in counts], out_off, max(sum(counts), 1)
    fmaps = {tuple(s[:3]) for s in anchor_shapes}
    if len(fmaps) != 1:
        raise ValueError(f"single-head target layout needs one feature map size for every anchor class, got {sorted(fmaps)}")
    locs = int(np.prod(next(iter(fmaps))))
    per_loc = [n // locs if locs else 1 for n in counts]
    out_off = [int(x) for x in np.cumsum([0] + per_loc[:-1])]
    return [max(r, 1) for r in per_loc], out_off, max(sum(per_loc), 1)


def code_size_of(anchor_dim, gt_box_dim, sincos):
    """width of ResidualCoder.encode_torch's output: 6 + the angle columns + zip(gt extras, anchor extras)"""
    return 6 + (2 if sincos else 1) + max(min(anchor_dim, gt_box_dim) - 7, 0)


def assign(anchors, gt_boxes_with_classes, class_of_id, per_loc, out_off, a_total, matched, unmatched, remap, code_size,
           sincos=False, norm_by_num_examples=False, gt_boxes_enlarged=None):
    """anchors: per-class contiguous (n_k, D) float32 device tensors in output order; gt_boxes_with_classes (B, M, C) float32
    [box | class id]; gt_boxes_enlarged: None or the same shape (its boxes are the ones encoded).
    -> labels (B, N) int32, targets (B, N, code_size) float32, weights (B, N) float32, N = sum n_k."""
    K = len(anchors)
    if not 0 < K <= MAX_CLASSES:
        raise _lib.LidarHipError(f"anchor_assign: 1..{MAX_CLASSES} anchor classes, got {K}")
    _lib.require_cuda(gt_boxes_with_classes, gt_boxes_enlarged, *anchors)
    gt = gt_boxes_with_classes
    if gt.dtype != torch.float32 or gt.dim() != 3 or gt.shape[2] < 8:
        raise _lib.LidarHipError(f"anchor_assign: gt_boxes must be float32 (B, M, >= 8), got {gt.dtype} {tuple(gt.shape)}")
    if gt_boxes_enlarged is not None and (gt_boxes_enlarged.shape != gt.shape or gt_boxes_enlarged.dtype != torch.float32):
        raise _lib.LidarHipError("anchor_assign: gt_boxes_enlarged must match gt_boxes in shape and dtype")
    D = anchors[0].shape[-1]
    for a in anchors:
        if a.dim() != 2 or a.shape[1] != D or a.dtype != torch.float32 or a.device != gt.device:
            raise _lib.LidarHipError("anchor_assign: anchors must be (n_k, D) float32 tensors on the gt boxes' device")
    if D < 7 or code_size != code_size_of(D, gt.shape[2] - 1, sincos) or code_size > MAX_CODE:
        raise _lib.LidarHipError(f"anchor_assign: code_size {code_size} does not match the encoding of {D}-column anchors and "
                                 f"{gt.shape[2] - 1}-column boxes (sincos={bool(sincos)})")
    B, M, gt_cols = (int(x) for x in gt.shape)
    N = sum(int(a.shape[0]) for a in anchors)
    dev = gt.device
    labels = torch.empty((B, N), dtype=torch.int32, device=dev)
    targets = torch.empty((B, N, code_size), dtype=torch.float32, device=dev)
    weights = torch.empty((B, N), dtype=torch.float32, device=dev)
    if B == 0 or N == 0:
        return labels, targets, weights
    L = _lib.lib()
    nbytes = L.lidar_anchor_assign_workspace_bytes(B, M, K)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    ll = lambda v: (C.c_longlong * K)(*[int(x) for x in v])   # noqa: E731
    status = L.lidar_anchor_assign(
        (C.c_void_p * K)(*[a.data_ptr() for a in anchors]), ll([a.shape[0] for a in anchors]), ll(per_loc), ll(out_off),
        _lib.host_f32(matched), _lib.host_f32(unmatched), _lib.host_i32(remap), K, int(D), int(a_total),
        (C.c_byte * NUM_IDS)(*[int(x) for x in class_of_id]), _lib.ptr(gt), _lib.ptr(gt_boxes_enlarged), B, M, gt_cols,
        int(code_size), int(bool(sincos)), int(bool(norm_by_num_examples)), _lib.ptr(labels), _lib.ptr(targets),
        _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(status, "lidar_anchor_assign")
    return labels, targets, weights
