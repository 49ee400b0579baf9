"""Host side of csrc/roi_loss.hip: the RoI heads' second-stage loss (RoIHeadTemplate.get_loss,
pcdet/models/roi_heads/roi_head_template.py:133-233) as one fused forward launch and a scale-and-store backward.

`spec_from_cfg` reads the loss settings of a ROI_HEAD config once and refuses what the kernel does not cover; `roi_head_loss`
returns (cls, reg, corner) as 0-dim device tensors, differentiable with respect to rcnn_cls and rcnn_reg, plus the 5-float device
record {cls, reg, corner, fg_sum, n_valid}.  The workspace comes from torch's caching allocator; nothing synchronises with the
host."""
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import LIMITS, cfg_get

MAX_SAMPLES, MAX_ROWS = LIMITS["LIDAR_ROI_LOSS_MAX_SAMPLES"], LIMITS["LIDAR_ROI_LOSS_MAX_ROWS"]


@dataclass(frozen=True)
class RoILossSpec:
    cls_weight: float
    reg_weight: float
    corner_weight: float
    code_weights: tuple
    corner: bool


def spec_from_cfg(model_cfg):
    """model_cfg: a ROI_HEAD config (LOSS_CONFIG; TARGET_CONFIG.BOX_CODER / BOX_CODER_CONFIG / REG_TRACKING_INFO when it has a
    TARGET_CONFIG).  NotImplementedError for what the kernel does not cover: the caller keeps a torch formulation for those."""
    loss_cfg = cfg_get(model_cfg, "LOSS_CONFIG")
    if loss_cfg is None:
        raise ValueError("roi_head_loss: the config has no LOSS_CONFIG")
    cls_loss, reg_loss = cfg_get(loss_cfg, "CLS_LOSS"), cfg_get(loss_cfg, "REG_LOSS")
    if cls_loss != "BinaryCrossEntropy":
        raise NotImplementedError(f"roi_head_loss: CLS_LOSS {cls_loss!r} is not supported (BinaryCrossEntropy)")
    if reg_loss != "smooth-l1":
        raise NotImplementedError(f"roi_head_loss: REG_LOSS {reg_loss!r} is not supported (smooth-l1)")
    tcfg = cfg_get(model_cfg, "TARGET_CONFIG") or {}
    coder = cfg_get(tcfg, "BOX_CODER", "ResidualCoder")
    coder_cfg = cfg_get(tcfg, "BOX_CODER_CONFIG") or {}
    if coder != "ResidualCoder" or cfg_get(coder_cfg, "encode_angle_by_sincos", False) or int(cfg_get(coder_cfg, "code_size", 7)) != 7:
        raise NotImplementedError(f"roi_head_loss: box coder {coder!r} {dict(coder_cfg)} is not supported (plain ResidualCoder, code size 7)")
    if cfg_get(tcfg, "REG_TRACKING_INFO", False):
        raise NotImplementedError("roi_head_loss: REG_TRACKING_INFO is not supported")
    lw = cfg_get(loss_cfg, "LOSS_WEIGHTS")
    code_weights = tuple(float(x) for x in lw["code_weights"])
    if len(code_weights) != 7:
        raise NotImplementedError(f"roi_head_loss: {len(code_weights)} code weights for a code size of 7")
    corner = bool(cfg_get(loss_cfg, "CORNER_LOSS_REGULARIZATION", False))
    return RoILossSpec(cls_weight=float(lw["rcnn_cls_weight"]), reg_weight=float(lw["rcnn_reg_weight"]),
                       corner_weight=float(lw["rcnn_corner_weight"]) if corner else 0.0, code_weights=code_weights, corner=corner)


def supported(batch, roi_per_image, roi_dim=7, gt_dim=8, reg_dim=7, cls_dim=1):
    """pure host: the shapes the kernel takes"""
    return bool(_lib.lib().lidar_roi_loss_supported(int(batch), int(roi_per_image), int(roi_dim), int(gt_dim), int(reg_dim), int(cls_dim)))


def workspace_bytes(batch, roi_per_image):
    """the device workspace one call takes (pure host query)"""
    return int(_lib.lib().lidar_roi_loss_workspace_bytes(int(batch), int(roi_per_image)))


def _host_args(spec):
    return (_lib.host_f32([spec.cls_weight, spec.reg_weight, spec.corner_weight]), _lib.host_f32(spec.code_weights),
            1 if spec.corner else 0)


class _RoILoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, B, P, rois, gt, gt_src, mask, labels, rcnn_cls, rcnn_reg):
        L = _lib.lib()
        dev = rcnn_cls.device
        ws = torch.empty(max(int(L.lidar_roi_loss_workspace_bytes(B, P)), 1), dtype=torch.uint8, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        _lib.check(L.lidar_roi_loss_forward(_lib.ptr(rcnn_cls), _lib.ptr(rcnn_reg), _lib.ptr(rois), _lib.ptr(gt), _lib.ptr(gt_src),
                                            _lib.ptr(mask), _lib.ptr(labels), B, P, *_host_args(spec), _lib.ptr(out), _lib.ptr(ws),
                                            ws.numel(), _lib.stream()), "lidar_roi_loss_forward")
        ctx.spec, ctx.shape = spec, (B, P)
        ctx.save_for_backward(rois, gt, gt_src, mask, labels, rcnn_cls, rcnn_reg, ws)
        return out

    @staticmethod
    def backward(ctx, grad):      # grad (5): the kernel reads the upstream gradients of cls, reg, corner; the counts carry none
        *_inputs, rcnn_cls, rcnn_reg, ws = ctx.saved_tensors
        B, P = ctx.shape
        need_cls, need_reg = ctx.needs_input_grad[8], ctx.needs_input_grad[9]
        d_cls = torch.empty_like(rcnn_cls) if need_cls else None
        d_reg = torch.empty_like(rcnn_reg) if need_reg else None
        grad = grad.contiguous()
        _lib.check(_lib.lib().lidar_roi_loss_backward(B, P, *_host_args(ctx.spec), _lib.ptr(grad), _lib.ptr(d_cls), _lib.ptr(d_reg),
                                                      _lib.ptr(ws), ws.numel(), _lib.stream()), "lidar_roi_loss_backward")
        return (None,) * 8 + (d_cls, d_reg)


def roi_head_loss(rcnn_cls, rcnn_reg, targets_dict, spec):
    """-> (cls, reg, corner, stats): the three weighted terms as 0-dim fp32 device tensors (reg WITHOUT the corner term; the
    reference's rcnn_loss_reg is reg + corner) and the device record stats = [cls, reg, corner, fg_sum, n_valid].

    rcnn_cls (B * P, 1) and rcnn_reg (B * P, 7) fp32; targets_dict as the target layer writes it: rois (B, P, 7), gt_of_rois /
    gt_of_rois_src (B, P, 8), reg_valid_mask (B, P) int64, rcnn_cls_labels (B, P) fp32.  The inputs are never written (the
    reference's encode_torch clamps gt_of_rois[..., 3:6] in place)."""
    rois, gt, gt_src = targets_dict["rois"], targets_dict["gt_of_rois"], targets_dict["gt_of_rois_src"]
    mask, labels = targets_dict["reg_valid_mask"], targets_dict["rcnn_cls_labels"]
    if rois.dim() != 3:
        _lib.fail("roi_head_loss", f"rois must be (B, P, 7), got {tuple(rois.shape)}")
    B, P = int(rois.shape[0]), int(rois.shape[1])
    n = B * P
    if rcnn_cls.dim() != 2 or rcnn_reg.dim() != 2 or rcnn_cls.shape[0] != n or rcnn_reg.shape[0] != n:
        _lib.fail("roi_head_loss", f"rcnn_cls / rcnn_reg must be ({n}, 1) / ({n}, 7), got {tuple(rcnn_cls.shape)} / {tuple(rcnn_reg.shape)}")
    if gt.dim() != 3 or tuple(gt.shape[:2]) != (B, P) or gt_src.shape != gt.shape:
        _lib.fail("roi_head_loss", f"gt_of_rois / gt_of_rois_src must be ({B}, {P}, 8), got {tuple(gt.shape)} / {tuple(gt_src.shape)}")
    if not supported(B, P, rois.shape[2], gt.shape[2], rcnn_reg.shape[1], rcnn_cls.shape[1]):
        _lib.fail("roi_head_loss", f"supported: rois (B, P, 7), gts (B, P, 8), rcnn_reg (n, 7), rcnn_cls (n, 1), 1 <= P <= {MAX_SAMPLES}, B * P <= "
                  f"{MAX_ROWS}; got rois {tuple(rois.shape)}, gts {tuple(gt.shape)}, rcnn_reg {tuple(rcnn_reg.shape)}, rcnn_cls "
                  f"{tuple(rcnn_cls.shape)}")
    if tuple(mask.shape) != (B, P) or mask.dtype != torch.int64:
        _lib.fail("roi_head_loss", f"reg_valid_mask must be int64 ({B}, {P}), got {mask.dtype} {tuple(mask.shape)}")
    if tuple(labels.shape) != (B, P):
        _lib.fail("roi_head_loss", f"rcnn_cls_labels must be ({B}, {P}), got {tuple(labels.shape)}")
    if labels.dtype == torch.int64:      # CLS_SCORE_TYPE cls: the target layer returns the 1 / 0 / -1 labels as int64, like the reference
        labels = labels.to(torch.float32)
    for name, t in [("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg), ("rois", rois), ("gt_of_rois", gt), ("gt_of_rois_src", gt_src),
                    ("rcnn_cls_labels", labels)]:
        if t.dtype != torch.float32:
            _lib.fail("roi_head_loss", f"{name} must be float32, got {t.dtype}")
    rois, gt, gt_src, mask, labels = (t.detach().contiguous() for t in (rois, gt, gt_src, mask, labels))
    rcnn_cls, rcnn_reg = rcnn_cls.contiguous(), rcnn_reg.contiguous()
    _lib.require_cuda(rcnn_cls, rcnn_reg, rois, gt, gt_src, mask, labels, allow=(torch.int64,))
    out = _RoILoss.apply(spec, B, P, rois, gt, gt_src, mask, labels, rcnn_cls, rcnn_reg)
    return out[0], out[1], out[2], out.detach()
