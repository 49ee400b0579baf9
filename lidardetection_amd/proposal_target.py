"""Host side of csrc/proposal_target.hip: second-stage RoI target assignment (ProposalTargetLayer,
pcdet/models/roi_heads/target_assigner/proposal_target_layer.py, plus the canonical transform of RoIHeadTemplate.assign_targets,
pcdet/models/roi_heads/roi_head_template.py:101-131) for a whole batch in one launch.

The quotas that the reference computes with Python double arithmetic are computed here the same way; a call allocates the outputs
from torch's caching allocator, launches on the current stream and never synchronises.  The kernel draws nothing: the caller passes
`fg_keys` (B, R) and `draws` (B, ROI_PER_IMAGE) in [0, 1) (see include/lidar_hip.h for the contract)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LIMITS

MAX_ROIS, MAX_GT = LIMITS["LIDAR_PROPOSAL_TARGET_MAX_ROIS"], LIMITS["LIDAR_PROPOSAL_TARGET_MAX_GT"]
MAX_SAMPLES, MAX_DIM = LIMITS["LIDAR_PROPOSAL_TARGET_MAX_SAMPLES"], LIMITS["LIDAR_PROPOSAL_TARGET_MAX_DIM"]
CLS_SCORE_TYPES = {"cls": 0, "roi_iou": 1}


def fg_rois_per_image(fg_ratio, roi_per_image):
    """proposal_target_layer.py:129"""
    return int(np.round(fg_ratio * roi_per_image))


def hard_quota_table(hard_bg_ratio, roi_per_image):
    """hard_quota[n] = int(n * HARD_BG_RATIO) for n = 0..ROI_PER_IMAGE (proposal_target_layer.py:177, Python doubles)"""
    return [int(n * hard_bg_ratio) for n in range(int(roi_per_image) + 1)]


def assign(rois, roi_scores, roi_labels, gt_boxes, fg_keys, draws, roi_per_image, fg_ratio, reg_fg_thresh, cls_fg_thresh,
           cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio, by_class=False, cls_score_type="roi_iou", gt_boxes_enlarged=None):
    """rois (B, R, D) f32, roi_scores (B, R) f32, roi_labels (B, R) i64, gt_boxes (B, M, D + 1) f32 [box | class id],
    fg_keys (B, R) f32, draws (B, roi_per_image) f32 -> dict of device tensors, P = roi_per_image:
    rois (B, P, D), gt_of_rois / gt_of_rois_src (B, P, D + 1), gt_iou_of_rois, roi_scores, rcnn_cls_labels (B, P) f32,
    roi_labels, reg_valid_mask (B, P) i64, sampled_inds (B, P) i32, frame_status (B,) i32, max_overlaps (B, R) f32,
    gt_assignment (B, R) i32."""
    if cls_score_type not in CLS_SCORE_TYPES:
        _lib.fail("proposal_target", f"CLS_SCORE_TYPE must be one of {sorted(CLS_SCORE_TYPES)}, got {cls_score_type!r}")
    if rois.dim() != 3 or rois.dtype != torch.float32:
        _lib.fail("proposal_target", f"rois must be float32 (B, R, D), got {rois.dtype} {tuple(rois.shape)}")
    B, R, D = (int(x) for x in rois.shape)
    P = int(roi_per_image)
    if gt_boxes.dim() != 3 or gt_boxes.dtype != torch.float32 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != D + 1:
        _lib.fail("proposal_target", f"gt_boxes must be float32 ({B}, M, {D + 1}), got {gt_boxes.dtype} {tuple(gt_boxes.shape)}")
    M = int(gt_boxes.shape[1])
    if gt_boxes_enlarged is not None and (gt_boxes_enlarged.shape != gt_boxes.shape or gt_boxes_enlarged.dtype != torch.float32):
        _lib.fail("proposal_target", f"gt_boxes_enlarged must match gt_boxes {tuple(gt_boxes.shape)} float32, got {gt_boxes_enlarged.dtype} "
                  f"{tuple(gt_boxes_enlarged.shape)}")
    for name, t, shape, dtype in [("roi_scores", roi_scores, (B, R), torch.float32), ("roi_labels", roi_labels, (B, R), torch.int64),
                                  ("fg_keys", fg_keys, (B, R), torch.float32), ("draws", draws, (B, P), torch.float32)]:
        if tuple(t.shape) != shape or t.dtype != dtype:
            _lib.fail("proposal_target", f"{name} must be {dtype} {shape}, got {t.dtype} {tuple(t.shape)}")
    if not (1 <= R <= MAX_ROIS and 1 <= M <= MAX_GT and 1 <= P <= MAX_SAMPLES and 7 <= D <= MAX_DIM):
        _lib.fail("proposal_target", f"supported: 1 <= R <= {MAX_ROIS}, 1 <= M <= {MAX_GT}, 1 <= ROI_PER_IMAGE <= {MAX_SAMPLES}, "
                  f"7 <= D <= {MAX_DIM}; got R {R}, M {M}, ROI_PER_IMAGE {P}, D {D}")
    fg_n = fg_rois_per_image(fg_ratio, P)
    if not 0 <= fg_n <= P or not 0.0 <= hard_bg_ratio <= 1.0:
        _lib.fail("proposal_target", f"FG_RATIO {fg_ratio} / HARD_BG_RATIO {hard_bg_ratio} must lie in [0, 1]")
    _lib.require_cuda(rois, roi_scores, roi_labels, gt_boxes, gt_boxes_enlarged, fg_keys, draws, allow=(torch.int64,))
    dev = rois.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = {
        "rois": torch.empty((B, P, D), **f32), "gt_of_rois": torch.empty((B, P, D + 1), **f32),
        "gt_of_rois_src": torch.empty((B, P, D + 1), **f32), "gt_iou_of_rois": torch.empty((B, P), **f32),
        "roi_scores": torch.empty((B, P), **f32), "roi_labels": torch.empty((B, P), dtype=torch.int64, device=dev),
        "reg_valid_mask": torch.empty((B, P), dtype=torch.int64, device=dev), "rcnn_cls_labels": torch.empty((B, P), **f32),
        "sampled_inds": torch.empty((B, P), dtype=torch.int32, device=dev),
        "frame_status": torch.empty((B,), dtype=torch.int32, device=dev), "max_overlaps": torch.empty((B, R), **f32),
        "gt_assignment": torch.empty((B, R), dtype=torch.int32, device=dev),
    }
    if B == 0:
        return out
    status = _lib.lib().lidar_proposal_target(
        _lib.ptr(rois), _lib.ptr(roi_scores), _lib.ptr(roi_labels), _lib.ptr(gt_boxes), _lib.ptr(gt_boxes_enlarged), B, R, M, D, P,
        fg_n, _lib.host_i32(hard_quota_table(hard_bg_ratio, P)), int(bool(by_class)), CLS_SCORE_TYPES[cls_score_type],
        float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh), float(cls_bg_thresh_lo),
        float(cls_fg_thresh - cls_bg_thresh), _lib.ptr(fg_keys), _lib.ptr(draws), _lib.ptr(out["rois"]), _lib.ptr(out["gt_of_rois"]),
        _lib.ptr(out["gt_of_rois_src"]), _lib.ptr(out["gt_iou_of_rois"]), _lib.ptr(out["roi_scores"]), _lib.ptr(out["roi_labels"]),
        _lib.ptr(out["reg_valid_mask"]), _lib.ptr(out["rcnn_cls_labels"]), _lib.ptr(out["sampled_inds"]),
        _lib.ptr(out["frame_status"]), _lib.ptr(out["max_overlaps"]), _lib.ptr(out["gt_assignment"]), _lib.stream())
    _lib.check(status, "lidar_proposal_target")
    return out
