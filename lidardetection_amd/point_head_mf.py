"""Host side of csrc/point_head_mf.hip: the multi-frame supervision of tools/cfgs/livox_models/pv_rcnn_multiframe.yaml, where every
gt carries its pose in each of the S stacked sweeps (locations (B, M, S, 3), rotations_y (B, M, S)).

`assign_point_targets_mf` is PointHeadSimpleMultiFrame.assign_targets (pcdet/models/dense_heads/point_head_simple_multiframe.py:
23-56) as one launch; `point_head_loss_mf` its get_cls_layer_loss (:58-90) as two forward launches and one backward launch,
differentiable with respect to the logits; `enlarged_gt_boxes` the USE_MULTIFRAME_ENLARGED_GT_BOXES block of AnchorHeadSingle.forward
(pcdet/models/dense_heads/anchor_head_single.py:61-89), whose result anchor_assign and proposal_target take as gt_boxes_enlarged.
The config is read by point_head.spec_from_cfg (this head has no box term, so the yaml's LOSS_REG: smooth-l1 is accepted).
Outputs and the workspace come from torch's caching allocator; nothing synchronises with the host."""
import torch

from . import _lib
from ._lib import LIMITS
from .point_head import MAX_BATCH, MAX_GT, MAX_POINTS, PointHeadSpec, spec_from_cfg  # noqa: F401  (re-exported)

MAX_FRAMES, MAX_CLASS = LIMITS["LIDAR_POINT_HEAD_MF_MAX_FRAMES"], LIMITS["LIDAR_POINT_HEAD_MF_MAX_CLASS"]


def supported(n, batch, m, stack_frame_size, num_class=1):
    """pure host: the shapes the kernels take"""
    return bool(_lib.lib().lidar_point_head_mf_supported(int(n), int(batch), int(m), int(stack_frame_size), int(num_class)))


def workspace_bytes(n):
    """the device workspace one loss call takes (pure host query)"""
    return int(_lib.lib().lidar_point_loss_mf_ws_bytes(int(n)))


def _check_poses(what, gt_boxes, locations, rotations_y):
    """-> (B, M, S) of gt_boxes (B, M, 8), locations (B, M, S, 3) and rotations_y (B, M, S) or None"""
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8:
        _lib.fail(what, f"gt_boxes must be (B, M, 8), got {tuple(gt_boxes.shape)}")
    B, M = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    if locations.dim() != 4 or tuple(locations.shape[:2]) != (B, M) or locations.shape[3] != 3:
        _lib.fail(what, f"locations must be ({B}, {M}, S, 3), got {tuple(locations.shape)}")
    S = int(locations.shape[2])
    if rotations_y is not None and tuple(rotations_y.shape) != (B, M, S):
        _lib.fail(what, f"rotations_y must be ({B}, {M}, {S}), got {tuple(rotations_y.shape)}")
    for name, t in (("gt_boxes", gt_boxes), ("locations", locations), ("rotations_y", rotations_y)):
        if t is not None and t.dtype != torch.float32:
            _lib.fail(what, f"{name} must be float32, got {t.dtype}")
    return B, M, S


def assign_point_targets_mf(points, gt_boxes, locations, rotations_y, spec):
    """points (N, 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) [box7 | class], locations (B, M, S, 3), rotations_y (B, M, S), fp32 on
    the device -> {point_cls_labels: a list of S (N,) int64 tensors (column views of the stacked tensor), point_cls_labels_stacked
    (N, S) int64, point_box_idx (N, S) int32, the owner gt row per frame (-1: none)}.  Column s is what
    point_head.assign_point_targets gives for gt_boxes with the centre and heading of frame s.  One launch, no host
    synchronisation; the inputs are never written."""
    what = "assign_point_targets_mf"
    if points.dim() != 2 or points.shape[1] != 4:
        _lib.fail(what, f"points must be (N, 4), got {tuple(points.shape)}")
    B, M, S = _check_poses(what, gt_boxes, locations, rotations_y)
    if points.dtype != torch.float32:
        _lib.fail(what, f"points must be float32, got {points.dtype}")
    N = int(points.shape[0])
    if not supported(N, B, M, S, spec.num_class):
        _lib.fail(what, f"supported: N <= {MAX_POINTS}, 1 <= B <= {MAX_BATCH}, M <= {MAX_GT}, 1 <= S <= {MAX_FRAMES}, num_class <= "
                  f"{MAX_CLASS}; got points {tuple(points.shape)}, locations {tuple(locations.shape)}, num_class {spec.num_class}")
    points, gt_boxes = points.detach().contiguous(), gt_boxes.detach().contiguous()
    locations, rotations_y = locations.detach().contiguous(), rotations_y.detach().contiguous()
    _lib.require_cuda(points, gt_boxes, locations, rotations_y)
    labels = torch.empty((N, S), dtype=torch.int64, device=points.device)
    owner = torch.empty((N, S), dtype=torch.int32, device=points.device)
    _lib.check(_lib.lib().lidar_point_targets_mf(_lib.ptr(points), N, _lib.ptr(gt_boxes), _lib.ptr(locations), _lib.ptr(rotations_y),
                                                 B, M, S, _lib.host_f32(spec.extra_width), spec.num_class, _lib.ptr(labels),
                                                 _lib.ptr(owner), _lib.stream()), "lidar_point_targets_mf")
    return {"point_cls_labels": list(labels.unbind(dim=1)), "point_cls_labels_stacked": labels, "point_box_idx": owner}


class _PointLossMF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, frames, labels, cls_preds):
        L = _lib.lib()
        n = int(labels.shape[0])
        ws = torch.empty(max(int(L.lidar_point_loss_mf_ws_bytes(n)), 1), dtype=torch.uint8, device=labels.device)
        out = torch.empty(2, dtype=torch.float32, device=labels.device)
        _lib.check(L.lidar_point_loss_mf_forward(_lib.ptr(cls_preds), _lib.ptr(labels), n, frames, spec.num_class, spec.cls_weight,
                                                 _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()), "lidar_point_loss_mf_forward")
        ctx.spec, ctx.frames = spec, frames
        ctx.save_for_backward(labels, cls_preds, ws)
        return out

    @staticmethod
    def backward(ctx, grad):      # grad (2): the kernel reads the upstream gradient of cls; the count carries none
        labels, cls_preds, ws = ctx.saved_tensors
        if not ctx.needs_input_grad[3]:
            return None, None, None, None
        d = torch.empty_like(cls_preds)
        grad = grad.contiguous()
        _lib.check(_lib.lib().lidar_point_loss_mf_backward(_lib.ptr(cls_preds), _lib.ptr(labels), int(labels.shape[0]), ctx.frames,
                                                           ctx.spec.num_class, ctx.spec.cls_weight, _lib.ptr(grad), _lib.ptr(d),
                                                           _lib.ptr(ws), ws.numel(), _lib.stream()), "lidar_point_loss_mf_backward")
        return None, None, None, d


def point_head_loss_mf(cls_preds, targets, spec, stack_frame_size):
    """-> (cls, stats): the weighted classification term as a 0-dim fp32 device tensor, differentiable with respect to cls_preds,
    and the device record stats = [cls, pos_num].  cls_preds (N, stack_frame_size * num_class) fp32, frame s in columns
    [s * num_class, (s + 1) * num_class); targets as assign_point_targets_mf writes them: point_cls_labels_stacked (N, S) int64, or
    the reference's list of S (N,) tensors under point_cls_labels, which is stacked here."""
    what = "point_head_loss_mf"
    S = int(stack_frame_size)
    labels = targets.get("point_cls_labels_stacked")
    if labels is None:
        labels = torch.stack(list(targets["point_cls_labels"]), dim=-1)
    if labels.dim() != 2 or labels.shape[1] != S:
        _lib.fail(what, f"the labels must be (N, {S}) for stack_frame_size {S}, got {tuple(labels.shape)}")
    if labels.dtype != torch.int64:
        _lib.fail(what, f"point_cls_labels must be int64, got {labels.dtype}")
    n = int(labels.shape[0])
    if not supported(n, 1, 0, S, spec.num_class):
        _lib.fail(what, f"supported: N <= {MAX_POINTS}, 1 <= S <= {MAX_FRAMES}, num_class <= {MAX_CLASS}; got N {n}, S {S}, "
                  f"num_class {spec.num_class}")
    if cls_preds.numel() == n * S * spec.num_class:
        cls_preds = cls_preds.reshape(n, S * spec.num_class)
    if cls_preds.dim() != 2 or tuple(cls_preds.shape) != (n, S * spec.num_class) or cls_preds.dtype != torch.float32:
        _lib.fail(what, f"point_cls_preds must be float32 ({n}, {S * spec.num_class}), got {cls_preds.dtype} {tuple(cls_preds.shape)}")
    labels, cls_preds = labels.detach().contiguous(), cls_preds.contiguous()
    _lib.require_cuda(labels, cls_preds, allow=(torch.int64,))
    out = _PointLossMF.apply(spec, S, labels, cls_preds)
    return out[0], out.detach()


def enlarged_gt_boxes(gt_boxes, locations, rotations_y=None):
    """gt_boxes (B, M, 8) [box7 | class], locations (B, M, S, 3) fp32 on the device -> gt_boxes_enlarged (B, M, 8): each gt with
    its length and width replaced by the extent, in its own frame, of its box placed at every one of its S locations
    (anchor_head_single.py:67-88).  rotations_y (B, M, S) is accepted because the reference takes it, and is NOT used: the reference
    writes it into the class column of its working copy, which the corner computation never reads, so every frame's box is turned by
    the gt's own heading.  One launch, no host synchronisation."""
    what = "enlarged_gt_boxes"
    if gt_boxes.dim() == 3 and gt_boxes.shape[2] != 8:
        _lib.fail(what, f"gt rows must have 8 columns [box7 | class], got {tuple(gt_boxes.shape)}: with more columns the reference's "
                  "[:, -2] is not the heading")
    B, M, S = _check_poses(what, gt_boxes, locations, rotations_y)
    if not supported(0, B, M, S, 1):
        _lib.fail(what, f"supported: 1 <= B <= {MAX_BATCH}, M <= {MAX_GT}, 1 <= S <= {MAX_FRAMES}; got locations {tuple(locations.shape)}")
    gt_boxes, locations = gt_boxes.detach().contiguous(), locations.detach().contiguous()
    _lib.require_cuda(gt_boxes, locations)
    out = torch.empty_like(gt_boxes)
    _lib.check(_lib.lib().lidar_multiframe_enlarged_boxes(_lib.ptr(gt_boxes), _lib.ptr(locations), B, M, 8, S, _lib.ptr(out),
                                                          _lib.stream()), "lidar_multiframe_enlarged_boxes")
    return out
