"""Host side of csrc/point_head.hip: the point heads' targets (PointHeadTemplate.assign_stack_targets with set_ignore_flag=True,
pcdet/models/dense_heads/point_head_template.py:49-129) as one launch, and their loss (get_cls_layer_loss / get_box_layer_loss /
get_part_layer_loss, :131-191) as two forward launches and one backward launch.

`spec_from_cfg` reads a POINT_HEAD config once and refuses what the kernels do not cover; `assign_point_targets` returns the
reference's targets_dict plus `point_box_idx`; `point_head_loss` returns (cls, box, part) as 0-dim device tensors, differentiable
with respect to the three prediction tensors, plus the 4-float device record {cls, box, part, pos_num}.  Outputs and the workspace
come from torch's caching allocator; nothing synchronises with the host."""
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import LIMITS, cfg_get

MAX_POINTS, MAX_BATCH, MAX_GT, MAX_CLASS, MAX_MEAN = (LIMITS["LIDAR_POINT_HEAD_MAX_" + k] for k in ("POINTS", "BATCH", "GT", "CLASS", "MEAN"))
CODE_SIZE = 8


@dataclass(frozen=True)
class PointHeadSpec:
    num_class: int
    extra_width: tuple          # GT_EXTRA_WIDTH
    box_coder: bool             # a PointResidualCoder is configured: the head has a box term
    mean_size: tuple            # ((dx, dy, dz), ...) per class, () without use_mean_size
    cls_weight: float
    box_weight: float
    part_weight: float
    code_weights: tuple         # 8 entries (ones where the config has no box term)


def spec_from_cfg(model_cfg, num_class):
    """model_cfg: a POINT_HEAD config (TARGET_CONFIG.GT_EXTRA_WIDTH / BOX_CODER / BOX_CODER_CONFIG, LOSS_CONFIG.LOSS_REG /
    LOSS_WEIGHTS).  NotImplementedError for what the kernels do not cover."""
    tcfg, loss_cfg = cfg_get(model_cfg, "TARGET_CONFIG"), cfg_get(model_cfg, "LOSS_CONFIG")
    if tcfg is None or loss_cfg is None:
        raise ValueError("point_head: the config needs TARGET_CONFIG and LOSS_CONFIG")
    num_class = int(num_class)
    if not 1 <= num_class <= MAX_CLASS:
        raise NotImplementedError(f"point_head: num_class {num_class} is not supported (1..{MAX_CLASS})")
    extra = tuple(float(x) for x in cfg_get(tcfg, "GT_EXTRA_WIDTH"))
    if len(extra) != 3:
        raise ValueError(f"point_head: GT_EXTRA_WIDTH needs 3 entries, got {extra}")
    lw = cfg_get(loss_cfg, "LOSS_WEIGHTS")
    coder = cfg_get(tcfg, "BOX_CODER", None)
    mean, code_weights = (), (1.0,) * CODE_SIZE
    if coder is not None:
        if coder != "PointResidualCoder":
            raise NotImplementedError(f"point_head: box coder {coder!r} is not supported (PointResidualCoder)")
        ccfg = cfg_get(tcfg, "BOX_CODER_CONFIG") or {}
        if int(cfg_get(ccfg, "code_size", CODE_SIZE)) != CODE_SIZE:
            raise NotImplementedError(f"point_head: code_size {cfg_get(ccfg, 'code_size')} is not supported ({CODE_SIZE})")
        if cfg_get(ccfg, "use_mean_size", True):
            mean = tuple(tuple(float(v) for v in row) for row in cfg_get(ccfg, "mean_size"))
            if not 1 <= len(mean) <= MAX_MEAN or any(len(r) != 3 or min(r) <= 0 for r in mean):
                raise NotImplementedError(f"point_head: mean_size must be 1..{MAX_MEAN} rows of 3 positive sizes, got {mean}")
        reg = cfg_get(loss_cfg, "LOSS_REG", None)
        if reg != "WeightedSmoothL1Loss":
            # point_head_template.py:23-33 maps every other value to F.smooth_l1_loss / F.l1_loss, which get_box_layer_loss then
            # calls with a `weights=` keyword those functions do not have: the reference raises a TypeError there
            raise NotImplementedError(f"point_head: LOSS_REG {reg!r} with a box term is not supported: the reference hands "
                                      "F.smooth_l1_loss / F.l1_loss a `weights=` argument they do not take and raises; use "
                                      "WeightedSmoothL1Loss")
        cw = cfg_get(lw, "code_weights", None)
        if cw is None or len(cw) != CODE_SIZE:
            raise NotImplementedError(f"point_head: the box term needs {CODE_SIZE} code_weights, got {cw}")
        code_weights = tuple(float(x) for x in cw)
    return PointHeadSpec(num_class=num_class, extra_width=extra, box_coder=coder is not None, mean_size=mean,
                         cls_weight=float(cfg_get(lw, "point_cls_weight")), box_weight=float(cfg_get(lw, "point_box_weight", 0.0)),
                         part_weight=float(cfg_get(lw, "point_part_weight", 0.0)), code_weights=code_weights)


def supported(n, batch, m, gt_dim=8, num_class=1, n_mean=0):
    """pure host: the shapes the kernels take"""
    return bool(_lib.lib().lidar_point_head_supported(int(n), int(batch), int(m), int(gt_dim), int(num_class), int(n_mean)))


def workspace_bytes(n):
    """the device workspace one loss call takes (pure host query)"""
    return int(_lib.lib().lidar_point_loss_ws_bytes(int(n)))


def assign_point_targets(points, gt_boxes, spec, ret_box_labels=False, ret_part_labels=False):
    """points (N, 4) [bs_idx, x, y, z] and gt_boxes (B, M, 8) [box7 | class] fp32 on the device -> the reference's targets_dict
    {point_cls_labels (N) int64, point_box_labels (N, 8) or None, point_part_labels (N, 3) or None} plus point_box_idx (N) int32,
    the owner gt row of each point (-1: none).  One launch, no host synchronisation; the inputs are never written."""
    what = "assign_point_targets"
    if points.dim() != 2 or points.shape[1] != 4:
        _lib.fail(what, f"points must be (N, 4), got {tuple(points.shape)}")
    if gt_boxes.dim() != 3:
        _lib.fail(what, f"gt_boxes must be (B, M, 8), got {tuple(gt_boxes.shape)}")
    if ret_box_labels and not spec.box_coder:
        _lib.fail(what, "box labels need a config with a PointResidualCoder")
    N, (B, M, D) = int(points.shape[0]), (int(s) for s in gt_boxes.shape)
    n_mean = len(spec.mean_size)
    if not supported(N, B, M, D, spec.num_class, n_mean):
        _lib.fail(what, f"supported: N <= {MAX_POINTS}, 1 <= B <= {MAX_BATCH}, M <= {MAX_GT}, gt rows of 8 columns, num_class <= "
                  f"{MAX_CLASS}; got points {tuple(points.shape)}, gt_boxes {tuple(gt_boxes.shape)}, num_class {spec.num_class}")
    for name, t in (("points", points), ("gt_boxes", gt_boxes)):
        if t.dtype != torch.float32:
            _lib.fail(what, f"{name} must be float32, got {t.dtype}")
    points, gt_boxes = points.detach().contiguous(), gt_boxes.detach().contiguous()
    _lib.require_cuda(points, gt_boxes)
    dev = points.device
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    owner = torch.empty(N, dtype=torch.int32, device=dev)
    box = torch.empty((N, CODE_SIZE), dtype=torch.float32, device=dev) if ret_box_labels else None
    part = torch.empty((N, 3), dtype=torch.float32, device=dev) if ret_part_labels else None
    mean = _lib.host_f32([v for row in spec.mean_size for v in row]) if n_mean else None
    flags = (1 if ret_box_labels else 0) | (2 if ret_part_labels else 0)
    _lib.check(_lib.lib().lidar_point_targets(_lib.ptr(points), N, _lib.ptr(gt_boxes), B, M, D, _lib.host_f32(spec.extra_width),
                                              spec.num_class, flags, mean, n_mean, _lib.ptr(labels), _lib.ptr(box), _lib.ptr(part),
                                              _lib.ptr(owner), _lib.stream()), "lidar_point_targets")
    return {"point_cls_labels": labels, "point_box_labels": box, "point_part_labels": part, "point_box_idx": owner}


def _host_args(spec):
    return _lib.host_f32([spec.cls_weight, spec.box_weight, spec.part_weight]), _lib.host_f32(spec.code_weights)


class _PointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, labels, box_labels, part_labels, cls_preds, box_preds, part_preds):
        L = _lib.lib()
        n = int(labels.shape[0])
        ws = torch.empty(max(int(L.lidar_point_loss_ws_bytes(n)), 1), dtype=torch.uint8, device=labels.device)
        out = torch.empty(4, dtype=torch.float32, device=labels.device)
        _lib.check(L.lidar_point_loss_forward(_lib.ptr(cls_preds), _lib.ptr(box_preds), _lib.ptr(part_preds), _lib.ptr(labels),
                                              _lib.ptr(box_labels), _lib.ptr(part_labels), n, spec.num_class, *_host_args(spec),
                                              _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()), "lidar_point_loss_forward")
        ctx.spec = spec
        ctx.save_for_backward(labels, box_labels, part_labels, cls_preds, box_preds, part_preds, ws)      # some are None
        return out

    @staticmethod
    def backward(ctx, grad):      # grad (4): the kernel reads the upstream gradients of cls, box, part; the count carries none
        labels, box_labels, part_labels, cls_preds, box_preds, part_preds, ws = ctx.saved_tensors
        need = ctx.needs_input_grad[4:7]
        d = [torch.empty_like(t) if (t is not None and nd) else None for t, nd in zip((cls_preds, box_preds, part_preds), need)]
        grad = grad.contiguous()
        _lib.check(_lib.lib().lidar_point_loss_backward(_lib.ptr(cls_preds), _lib.ptr(box_preds), _lib.ptr(part_preds),
                                                        _lib.ptr(labels), _lib.ptr(box_labels), _lib.ptr(part_labels),
                                                        int(labels.shape[0]), ctx.spec.num_class, *_host_args(ctx.spec),
                                                        _lib.ptr(grad), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(ws),
                                                        ws.numel(), _lib.stream()), "lidar_point_loss_backward")
        return (None,) * 4 + tuple(d)


def point_head_loss(cls_preds, box_preds, part_preds, targets, spec):
    """-> (cls, box, part, stats): the three weighted terms as 0-dim fp32 device tensors and the device record stats = [cls, box,
    part, pos_num].  cls_preds (N, num_class), box_preds (N, 8) or None, part_preds (N, 3) or None, fp32; targets as
    assign_point_targets writes them (point_cls_labels int64; the box / part labels of the terms that are present).  A term whose
    prediction is None is skipped and comes back as 0."""
    what = "point_head_loss"
    labels = targets["point_cls_labels"].reshape(-1)
    n = int(labels.shape[0])
    if labels.dtype != torch.int64:
        _lib.fail(what, f"point_cls_labels must be int64, got {labels.dtype}")
    if not supported(n, 1, 0, 8, spec.num_class, 0):
        _lib.fail(what, f"supported: N <= {MAX_POINTS}, num_class <= {MAX_CLASS}; got N {n}, num_class {spec.num_class}")
    box_labels = targets.get("point_box_labels") if box_preds is not None else None
    part_labels = targets.get("point_part_labels") if part_preds is not None else None
    if cls_preds is not None:
        cls_preds = cls_preds.reshape(-1, spec.num_class)
    for name, t, lab, width in (("point_cls_preds", cls_preds, labels, spec.num_class), ("point_box_preds", box_preds, box_labels, CODE_SIZE),
                                ("point_part_preds", part_preds, part_labels, 3)):
        if t is None:
            continue
        if lab is None:
            _lib.fail(what, f"{name} without its labels in the targets")
        if t.dim() != 2 or tuple(t.shape) != (n, width) or t.dtype != torch.float32:
            _lib.fail(what, f"{name} must be float32 ({n}, {width}), got {t.dtype} {tuple(t.shape)}")
        if lab is not labels and (tuple(lab.shape) != (n, width) or lab.dtype != torch.float32):
            _lib.fail(what, f"the labels of {name} must be float32 ({n}, {width}), got {lab.dtype} {tuple(lab.shape)}")
    cont = lambda t: None if t is None else t.contiguous()      # noqa: E731
    det = lambda t: None if t is None else t.detach().contiguous()      # noqa: E731
    labels, box_labels, part_labels = det(labels), det(box_labels), det(part_labels)
    cls_preds, box_preds, part_preds = cont(cls_preds), cont(box_preds), cont(part_preds)
    _lib.require_cuda(labels, box_labels, part_labels, cls_preds, box_preds, part_preds, allow=(torch.int64,))
    out = _PointLoss.apply(spec, labels, box_labels, part_labels, cls_preds, box_preds, part_preds)
    return out[0], out[1], out[2], out.detach()
