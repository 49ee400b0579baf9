"""Host side of csrc/anchor_loss.hip: the anchor heads' RPN loss (AnchorHeadTemplate.get_loss / AnchorHeadMulti.get_loss,
pcdet/models/dense_heads/anchor_head_template.py, anchor_head_multi.py:245-370) as one fused forward and one fused backward.

`spec_from_cfg` reads the loss settings of a dense-head config once and refuses what the kernels do not cover; `anchor_head_loss`
returns (cls_loss, loc_loss, dir_loss) as 0-dim device tensors, differentiable with respect to the predictions.  Per-head
prediction tensors go to the kernels as separate pointers (no cat); the workspace comes from torch's caching allocator; nothing
synchronises with the host."""
import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import cfg_get

MAX_HEADS = 16    # csrc/anchor_loss.hip: AL_MAX_HEADS
MAX_CODE = 16     # AL_MAX_CODE
MAX_COLS = 16     # AL_MAX_COLS: class columns of one head
MAX_BINS = 8      # AL_MAX_BINS
REG_LOSSES = {"WeightedSmoothL1Loss": 0, "WeightedL1Loss": 2}   # -> kernel flag


@dataclass(frozen=True)
class LossSpec:
    """What the loss reads off the dense-head config.  head_classes / head_class_offsets: per head, its class columns and its
    first one-hot column (SEPARATE_MULTIHEAD), or None for one head (template) / heads that each predict all num_class columns."""
    num_class: int
    multihead: bool
    separate: bool
    head_classes: tuple
    head_class_offsets: tuple
    cls_weight: float
    loc_weight: float
    dir_weight: float
    pos_cls_weight: float
    neg_cls_weight: float
    code_weights: tuple
    reg_loss: str
    use_dir: bool
    dir_offset: float
    num_dir_bins: int


def spec_from_cfg(model_cfg, num_class, head_num_classes=None):
    """model_cfg: a DENSE_HEAD config (LOSS_CONFIG, DIR_OFFSET, NUM_DIR_BINS, USE_DIRECTION_CLASSIFIER, USE_MULTIHEAD,
    SEPARATE_MULTIHEAD).  head_num_classes: AnchorHeadMulti's per-head class counts (rpn_heads[i].num_class); None for
    AnchorHeadTemplate.  Multi with SEPARATE_MULTIHEAD: head i compares its columns with one-hot columns sum(c[<i]) ..; without
    it every head predicts all num_class columns."""
    loss_cfg = cfg_get(model_cfg, "LOSS_CONFIG")
    lw = cfg_get(loss_cfg, "LOSS_WEIGHTS")
    reg = cfg_get(loss_cfg, "REG_LOSS_TYPE", None) or "WeightedSmoothL1Loss"
    if reg not in REG_LOSSES:
        raise NotImplementedError(f"anchor_head_loss: REG_LOSS_TYPE {reg!r} is not supported ({sorted(REG_LOSSES)})")
    if lw.get("code_weights") is None:
        raise ValueError("anchor_head_loss: LOSS_WEIGHTS needs code_weights (the reference's regression losses read them)")
    code_weights = tuple(float(x) for x in lw["code_weights"])
    if not 7 <= len(code_weights) <= MAX_CODE:
        raise NotImplementedError(f"anchor_head_loss: code size {len(code_weights)} outside 7..{MAX_CODE}")
    num_class = int(num_class)
    multihead = head_num_classes is not None
    separate = bool(cfg_get(model_cfg, "SEPARATE_MULTIHEAD", False)) if multihead else False
    if multihead:
        heads = [int(c) for c in head_num_classes]
        if separate:
            offs = [sum(heads[:i]) for i in range(len(heads))]
            if sum(heads) > num_class:
                raise ValueError(f"anchor_head_loss: heads' classes {heads} exceed num_class {num_class}")
        else:
            heads, offs = [num_class] * len(heads), [0] * len(heads)
        # anchor_head_multi.py:247-251: both weights when pos_cls_weight is given, else 1 and 1
        pos_w, neg_w = (float(lw["pos_cls_weight"]), float(lw["neg_cls_weight"])) if "pos_cls_weight" in lw else (1.0, 1.0)
    else:
        heads, offs, pos_w, neg_w = [num_class], [0], 1.0, 1.0
    if not 0 < len(heads) <= MAX_HEADS:
        raise NotImplementedError(f"anchor_head_loss: 1..{MAX_HEADS} heads, got {len(heads)}")
    if any(not 0 < c <= MAX_COLS for c in heads):
        raise NotImplementedError(f"anchor_head_loss: 1..{MAX_COLS} class columns per head, got {heads}")
    use_dir = bool(cfg_get(model_cfg, "USE_DIRECTION_CLASSIFIER", False))
    bins = int(cfg_get(model_cfg, "NUM_DIR_BINS", 2) or 0)
    if use_dir and not 0 < bins <= MAX_BINS:
        raise NotImplementedError(f"anchor_head_loss: NUM_DIR_BINS {bins} outside 1..{MAX_BINS}")
    return LossSpec(num_class=num_class, multihead=multihead, separate=separate, head_classes=tuple(heads),
                    head_class_offsets=tuple(offs), cls_weight=float(lw["cls_weight"]), loc_weight=float(lw["loc_weight"]),
                    dir_weight=float(lw.get("dir_weight", 0.0)) if use_dir else 0.0, pos_cls_weight=pos_w,
                    neg_cls_weight=neg_w, code_weights=code_weights, reg_loss=reg, use_dir=use_dir,
                    dir_offset=float(cfg_get(model_cfg, "DIR_OFFSET", 0.0) or 0.0), num_dir_bins=bins)


def _heads(x, name, B, n_heads, last):
    """a tensor or a list of per-head tensors in the reference's views -> per-head contiguous (B, n_h, last) fp32 tensors"""
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    if len(xs) != n_heads:
        raise _lib.LidarHipError(f"anchor_head_loss: {name}: {len(xs)} tensors for {n_heads} heads")
    out = []
    for t, c in zip(xs, last):
        if t.dtype != torch.float32:
            raise _lib.LidarHipError(f"anchor_head_loss: {name} must be float32 (the reference's dtype), got {t.dtype}")
        if t.shape[0] != B or t.numel() % (B * c):
            raise _lib.LidarHipError(f"anchor_head_loss: {name} {tuple(t.shape)} does not view as ({B}, -1, {c})")
        out.append(t.contiguous().view(B, -1, c))
    return out


class _AnchorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, labels, targets, anchors, *preds):
        H = meta["H"]
        cls, box, dirs = preds[:H], preds[H:2 * H], preds[2 * H:]
        L = _lib.lib()
        counts = (C.c_longlong * H)(*[int(t.shape[1]) for t in cls])
        dev = labels.device
        ws = torch.empty(max(int(L.lidar_anchor_loss_workspace_bytes(meta["B"], counts, H)), 1), dtype=torch.uint8, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        args = _abi_args(meta, cls, box, dirs, counts, labels, targets, anchors)
        _lib.check(L.lidar_anchor_loss_forward(*args, _lib.ptr(losses), _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "lidar_anchor_loss_forward")
        ctx.meta, ctx.counts = meta, counts
        ctx.save_for_backward(labels, targets, anchors, ws, *preds)
        return losses

    @staticmethod
    def backward(ctx, grad):
        meta, H = ctx.meta, ctx.meta["H"]
        labels, targets, anchors, ws, *preds = ctx.saved_tensors
        cls, box, dirs = preds[:H], preds[H:2 * H], preds[2 * H:]
        need = ctx.needs_input_grad[4:]
        grad = grad.contiguous()
        out = [torch.empty_like(t) if need[k] else None for k, t in enumerate(preds)]
        arr = lambda ts: (C.c_void_p * H)(*[t.data_ptr() if t is not None else None for t in ts]) if ts else None   # noqa: E731
        args = _abi_args(meta, cls, box, dirs, ctx.counts, labels, targets, anchors)
        _lib.check(_lib.lib().lidar_anchor_loss_backward(*args, _lib.ptr(grad), arr(out[:H]), arr(out[H:2 * H]),
                                                         arr(out[2 * H:]), _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "lidar_anchor_loss_backward")
        return (None, None, None, None, *out)


def _abi_args(meta, cls, box, dirs, counts, labels, targets, anchors):
    H, spec = meta["H"], meta["spec"]
    ptrs = lambda ts: (C.c_void_p * H)(*[t.data_ptr() for t in ts])   # noqa: E731
    code = len(spec.code_weights)
    weights = [spec.cls_weight, spec.loc_weight, spec.dir_weight, spec.pos_cls_weight, spec.neg_cls_weight, spec.dir_offset,
               2 * math.pi / spec.num_dir_bins if spec.num_dir_bins else 0.0]
    return (ptrs(cls), ptrs(box), ptrs(dirs) if dirs else None, counts, _lib.host_i32(meta["cols"]), _lib.host_i32(meta["offs"]),
            H, _lib.ptr(labels), _lib.ptr(targets), _lib.ptr(anchors), int(anchors.shape[-1]) if anchors is not None else 0,
            meta["B"], meta["N"], spec.num_class, code, spec.num_dir_bins if dirs else 0, _lib.host_f32(spec.code_weights),
            _lib.host_f32(weights), meta["flags"])


def anchor_head_loss(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, spec):
    """-> (cls_loss, loc_loss, dir_loss): 0-dim fp32 device tensors, each already weighted and divided by the batch size as the
    reference's get_cls_layer_loss / get_box_reg_layer_loss return them; dir_loss is 0 without direction predictions.

    cls_preds / box_preds / dir_cls_preds: a tensor, or a list with one tensor per head, in the reference's views (template:
    (B, H, W, A * C) or (B, N, C); multi: (B, n_h, c_h)); dir_cls_preds may be None.  box_cls_labels (B, N) int32,
    box_reg_targets (B, N, code_size) fp32 as the assigner writes them; anchors: the frame's N anchors in the same order
    (anything that views as (N, D)).  The template's add_sin_difference is always applied, the multi-head one only with
    direction predictions (anchor_head_multi.py:340-345)."""
    labels, targets = box_cls_labels, box_reg_targets
    if labels.dtype != torch.int32 or labels.dim() != 2:
        raise _lib.LidarHipError(f"anchor_head_loss: box_cls_labels must be (B, N) int32, got {labels.dtype} {tuple(labels.shape)}")
    B, N = (int(x) for x in labels.shape)
    code = len(spec.code_weights)
    if targets.dtype != torch.float32 or tuple(targets.shape) != (B, N, code):
        raise _lib.LidarHipError(f"anchor_head_loss: box_reg_targets must be ({B}, {N}, {code}) float32, got {targets.dtype} "
                                 f"{tuple(targets.shape)}")
    n_heads = len(cls_preds) if isinstance(cls_preds, (list, tuple)) else 1
    if spec.multihead:
        cols = list(spec.head_classes) if spec.separate else [spec.num_class] * n_heads
        offs = list(spec.head_class_offsets) if spec.separate else [0] * n_heads
        if len(cols) != n_heads:
            raise _lib.LidarHipError(f"anchor_head_loss: {n_heads} class-prediction heads for a spec of {len(cols)}")
    else:
        cols, offs = [spec.num_class], [0]
    cls = _heads(cls_preds, "cls_preds", B, n_heads, cols)
    box = _heads(box_preds, "box_preds", B, n_heads, [code] * n_heads)
    dirs = []
    if dir_cls_preds is not None:
        if not spec.num_dir_bins:
            raise _lib.LidarHipError("anchor_head_loss: direction predictions for a spec without NUM_DIR_BINS")
        dirs = _heads(dir_cls_preds, "dir_cls_preds", B, n_heads, [spec.num_dir_bins] * n_heads)
        if anchors is None or anchors.dtype != torch.float32 or anchors.dim() < 1 or anchors.shape[-1] < 7 or \
                anchors.numel() != N * anchors.shape[-1]:
            raise _lib.LidarHipError(f"anchor_head_loss: anchors must view as ({N}, >= 7) float32")
        anchors = anchors.contiguous()
        _lib.require_cuda(anchors)
    else:
        anchors = None
    _lib.require_cuda(labels, targets, *cls, *box, *dirs)
    if [t.shape[1] for t in box] != [t.shape[1] for t in cls] or (dirs and [t.shape[1] for t in dirs] != [t.shape[1] for t in cls]):
        raise _lib.LidarHipError("anchor_head_loss: the heads' class, box and direction predictions cover different anchors")
    if sum(int(t.shape[1]) for t in cls) != N:
        raise _lib.LidarHipError(f"anchor_head_loss: the heads cover {sum(int(t.shape[1]) for t in cls)} anchors, labels {N}")
    sin_diff = (not spec.multihead) or bool(dirs)
    flags = (1 if sin_diff else 0) | REG_LOSSES[spec.reg_loss] | (4 if dirs else 0)
    meta = dict(H=n_heads, B=B, N=N, spec=spec, cols=cols, offs=offs, flags=flags)
    losses = _AnchorLoss.apply(meta, labels.contiguous(), targets.contiguous(), anchors, *cls, *box, *dirs)
    return losses[0], losses[1], losses[2]


def workspace_bytes(batch, head_counts):
    """the device workspace one call takes (pure host query)"""
    H = len(head_counts)
    return int(_lib.lib().lidar_anchor_loss_workspace_bytes(int(batch), (C.c_longlong * H)(*[int(n) for n in head_counts]), H))
