"""Host side of csrc/atss_assign.hip: ATSS anchor target assignment (ATSSTargetAssigner,
pcdet/models/dense_heads/target_assigner/atss_target_assigner.py) for a whole batch and every anchor set in one call.

A call checks its arguments against the kernel's declared support (an unsupported one is an error before any launch), allocates
the outputs and a workspace from torch's caching allocator, launches on the current stream and never synchronises."""
import ctypes as C

import torch

from . import _lib
from .anchor_assign import code_size_of

MAX_SETS = 16         # anchor sets per call (csrc/atss_assign.hip: AT_MAX_SETS)
MIN_TOPK, MAX_TOPK = 2, 32   # TOPK 1 has no unbiased std (AT_MAX_TOPK)
MAX_GT = 256          # gt rows per frame (AT_MAX_GT)
MAX_CODE = 16         # code_size (AT_MAX_CODE)


def supported(counts, anchor_dim, gt_cols, code_size, sincos, topk, max_gt, match_height):
    """lidar_atss_assign_supported: pure host, no device needed"""
    K = len(counts)
    return bool(_lib.lib().lidar_atss_assign_supported((C.c_longlong * max(K, 1))(*[int(x) for x in counts]), K, int(anchor_dim),
                                                       int(gt_cols), int(code_size), int(sincos), int(topk), int(max_gt),
                                                       int(match_height)))


def workspace_bytes(batch, max_gt, num_sets, topk):
    return int(_lib.lib().lidar_atss_assign_workspace_bytes(int(batch), int(max_gt), int(num_sets), int(topk)))


def assign(anchors, gt_boxes_with_classes, topk, code_size, sincos=False, match_height=False):
    """anchors: per-set contiguous (n_k, D) float32 device tensors in output order; gt_boxes_with_classes (B, M, C) float32
    [box | class id].  -> labels (B, N) int32, targets (B, N, code_size) float32, weights (B, N) float32, N = sum n_k, the sets
    one after the other."""
    K = len(anchors)
    if not 0 < K <= MAX_SETS:
        raise _lib.LidarHipError(f"atss_assign: 1..{MAX_SETS} anchor sets, got {K}")
    _lib.require_cuda(gt_boxes_with_classes, *anchors)
    gt = gt_boxes_with_classes
    if gt.dtype != torch.float32 or gt.dim() != 3 or gt.shape[2] < 8:
        raise _lib.LidarHipError(f"atss_assign: gt_boxes must be float32 (B, M, >= 8), got {gt.dtype} {tuple(gt.shape)}")
    D = anchors[0].shape[-1]
    for a in anchors:
        if a.dim() != 2 or a.shape[1] != D or a.dtype != torch.float32 or a.device != gt.device:
            raise _lib.LidarHipError("atss_assign: anchors must be (n_k, D) float32 tensors on the gt boxes' device")
    B, M, gt_cols = (int(x) for x in gt.shape)
    counts = [int(a.shape[0]) for a in anchors]
    if D < 7 or code_size != code_size_of(D, gt_cols - 1, sincos) or code_size > MAX_CODE:
        raise _lib.LidarHipError(f"atss_assign: code_size {code_size} does not match the encoding of {D}-column anchors and "
                                 f"{gt_cols - 1}-column boxes (sincos={bool(sincos)})")
    if not supported(counts, D, gt_cols, code_size, bool(sincos), topk, M, bool(match_height)):
        raise _lib.LidarHipError(f"atss_assign: unsupported: TOPK {topk} (need {MIN_TOPK}..{MAX_TOPK} and <= every set's anchor "
                                 f"count, got {counts}), max_gt {M} (1..{MAX_GT})")
    N = sum(counts)
    dev = gt.device
    labels = torch.empty((B, N), dtype=torch.int32, device=dev)
    targets = torch.empty((B, N, code_size), dtype=torch.float32, device=dev)
    weights = torch.empty((B, N), dtype=torch.float32, device=dev)
    if B == 0:
        return labels, targets, weights
    L = _lib.lib()
    ws = torch.empty(max(workspace_bytes(B, M, K, topk), 1), dtype=torch.uint8, device=dev)
    status = L.lidar_atss_assign(
        (C.c_void_p * K)(*[a.data_ptr() for a in anchors]), (C.c_longlong * K)(*counts), K, int(D), _lib.ptr(gt), B, M, gt_cols,
        int(code_size), int(bool(sincos)), int(topk), int(bool(match_height)), _lib.ptr(labels), _lib.ptr(targets),
        _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(status, "lidar_atss_assign")
    return labels, targets, weights
