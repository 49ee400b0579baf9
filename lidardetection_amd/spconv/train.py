"""Train-mode BatchNorm1d + ReLU on sparse features, fused (csrc/bn_train.hip).

reference: pcdet/models/backbones_3d/spconv_backbone.py:7-26 (post_act_block: conv -> BatchNorm1d -> ReLU) and :29-65
(SparseBasicBlock: bn1 -> relu, bn2 -> += identity -> relu).

The features of a SparseConvTensor are an (N, C) matrix, which is the `rows x C` map the dense backbone's fused train-mode
BatchNorm + ReLU kernels take with one segment, rows = N and row stride C: fp64 fixed-order batch statistics, y = relu(bn(z)) in one
pass, the backward's ReLU mask recomputed from z (only z is saved), no float atomics and no host read.  The residual form
y = relu(bn(z) + r) is the same kernels with the residual added before the ReLU (lidar_bn_add_relu_train_*).

Opt-in: inside `with fused_bn_train():` a grad-mode SparseSequential runs every supported BatchNorm1d -> ReLU pair as the fused
call and SparseBasicBlock runs bn1 -> relu and bn2 -> += identity -> relu on them; outside it nothing changes.
"""
import contextlib
import ctypes as C

import torch
from torch import nn

from .. import _lib, workspace

_MAX_C = 1024         # csrc/bn_train.hip BT_MAX_C
_ENABLED = [False]


@contextlib.contextmanager
def fused_bn_train(enabled=True):
    """inside: grad-mode SparseSequential / SparseBasicBlock run their train-mode BatchNorm1d (+ residual) + ReLU on the fused kernels
    wherever bn_supported() holds and the tensor has at least 2 rows; anything else runs the modules as outside"""
    was = _ENABLED[0]
    _ENABLED[0] = bool(enabled)
    try:
        yield
    finally:
        _ENABLED[0] = was


def fused_bn_train_enabled():
    return _ENABLED[0]


def bn_supported(bn, channels=None):
    """the fused kernels take this BatchNorm1d: in training mode, affine, tracking running statistics with a numeric momentum
    (momentum=None's cumulative average stays on torch), C % 4 == 0 and 4 <= C <= 1024.  Pure host."""
    if not isinstance(bn, nn.BatchNorm1d):
        return False
    c = bn.num_features if channels is None else int(channels)
    return (bn.training and bn.affine and bn.track_running_stats and bn.running_mean is not None
            and bn.num_batches_tracked is not None and isinstance(bn.momentum, (int, float)) and not isinstance(bn.momentum, bool)
            and c == bn.num_features and c % 4 == 0 and 4 <= c <= _MAX_C)


def takes(bn, feats):
    """the fused route applies to module `bn` on the feature matrix `feats` (bn_supported, fp32 on the device, N >= 2)"""
    return (bn_supported(bn, feats.shape[1] if feats.dim() == 2 else -1) and feats.is_cuda and feats.dtype == torch.float32
            and feats.shape[0] >= 2 and bn.weight.is_cuda and bn.weight.dtype == torch.float32)


def _check_rows(what, z, r=None):
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.is_contiguous()):
        raise _lib.LidarHipError(f"{what}: expected a contiguous 2-d float32 CUDA (ROCm) matrix, got {z.dtype} {tuple(z.shape)} on {z.device}")
    n, c = z.shape
    if n < 2 or c % 4 or not 4 <= c <= _MAX_C:
        raise _lib.LidarHipError(f"{what}: needs at least 2 rows and a multiple of 4 channels in [4, {_MAX_C}], got {tuple(z.shape)}")
    if r is not None and not (r.is_cuda and r.dtype == torch.float32 and r.shape == z.shape and r.is_contiguous()):
        raise _lib.LidarHipError(f"{what}: the residual must be a contiguous float32 CUDA matrix of shape {tuple(z.shape)}")
    return n, c


def _seg(z, c):
    """the one-segment tables of lidar_bn_relu_train_*: (x, x_ld, x_off, seg_C) for the (N, c) matrix z"""
    return (C.c_void_p * 1)(z.data_ptr()), _lib.host_i32([c]), _lib.host_i32([0]), _lib.host_i32([c])


def bn_relu_rows_forward(z, gamma, beta, eps, residual=None):
    """y = relu(batch_norm(z, training=True) [+ residual]) for an (N, C) matrix -> (y, stats, scale_shift, batch_stats) as
    bev_train.bn_relu_forward returns them.  No host synchronisation."""
    n, c = _check_rows("bn_relu_rows_forward", z, residual)
    _lib.require_cuda(gamma, beta)
    if gamma.numel() != c or beta.numel() != c:
        raise _lib.LidarHipError(f"bn_relu_rows_forward: gamma / beta must hold {c} values")
    dev = z.device
    y = torch.empty_like(z)
    stats = torch.empty(2 * c, dtype=torch.float64, device=dev)
    scale_shift = torch.empty(2 * c, dtype=torch.float32, device=dev)
    batch_stats = torch.empty(3 * c, dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.lidar_bn_relu_train_workspace_bytes(n, c)
    ws = workspace.get("bn_train", wsb, dev)
    if residual is None:
        _lib.check(L.lidar_bn_relu_train_forward(1, *_seg(z, c), n,
                                                 _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(y), c, 0, _lib.ptr(stats),
                                                 _lib.ptr(scale_shift), _lib.ptr(batch_stats), _lib.ptr(ws), wsb, _lib.stream()),
                   "lidar_bn_relu_train_forward")
    else:
        _lib.check(L.lidar_bn_add_relu_train_forward(_lib.ptr(z), c, _lib.ptr(residual), c, c, n, _lib.ptr(gamma), _lib.ptr(beta),
                                                     float(eps), _lib.ptr(y), c, _lib.ptr(stats), _lib.ptr(scale_shift),
                                                     _lib.ptr(batch_stats), _lib.ptr(ws), wsb, _lib.stream()),
                   "lidar_bn_add_relu_train_forward")
    return y, stats, scale_shift, batch_stats


def bn_relu_rows_backward(z, grad_y, gamma, stats, scale_shift, residual=None):
    """the backward of bn_relu_rows_forward -> (dz, d_residual or None, d_gamma, d_beta)"""
    n, c = _check_rows("bn_relu_rows_backward", z, residual)
    g = grad_y.contiguous()
    if g.shape != z.shape or g.dtype != torch.float32 or not g.is_cuda:
        raise _lib.LidarHipError(f"bn_relu_rows_backward: the gradient must be a float32 CUDA matrix of shape {tuple(z.shape)}")
    _lib.require_cuda(gamma, scale_shift)
    dev = z.device
    dz = torch.empty_like(z)
    d_gamma = torch.empty(c, dtype=torch.float32, device=dev)
    d_beta = torch.empty(c, dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.lidar_bn_relu_train_workspace_bytes(n, c)
    ws = workspace.get("bn_train", wsb, dev)
    if residual is None:
        _lib.check(L.lidar_bn_relu_train_backward(1, *_seg(z, c), n,
                                                  _lib.ptr(g), c, 0, _lib.ptr(gamma), _lib.ptr(stats), _lib.ptr(scale_shift),
                                                  (C.c_void_p * 1)(dz.data_ptr()), _lib.ptr(d_gamma), _lib.ptr(d_beta), _lib.ptr(ws), wsb,
                                                  _lib.stream()), "lidar_bn_relu_train_backward")
        return dz, None, d_gamma, d_beta
    dr = torch.empty_like(z)
    _lib.check(L.lidar_bn_add_relu_train_backward(_lib.ptr(z), c, _lib.ptr(residual), c, c, n, _lib.ptr(g), c, _lib.ptr(gamma),
                                                  _lib.ptr(stats), _lib.ptr(scale_shift), _lib.ptr(dz), _lib.ptr(dr), c,
                                                  _lib.ptr(d_gamma), _lib.ptr(d_beta), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_add_relu_train_backward")
    return dz, dr, d_gamma, d_beta


class _BNReLURows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eps, gamma, beta, z):
        y, stats, scale_shift, batch_stats = bn_relu_rows_forward(z, gamma, beta, eps)
        ctx.save_for_backward(gamma, stats, scale_shift, z)            # z only: y and the ReLU mask are recomputed
        ctx.mark_non_differentiable(batch_stats)
        return y, batch_stats

    @staticmethod
    def backward(ctx, grad_y, _grad_stats):
        gamma, stats, scale_shift, z = ctx.saved_tensors
        dz, _, d_gamma, d_beta = bn_relu_rows_backward(z, grad_y, gamma, stats, scale_shift)
        need = ctx.needs_input_grad
        return None, d_gamma if need[1] else None, d_beta if need[2] else None, dz if need[3] else None


class _BNAddReLURows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eps, gamma, beta, z, r):
        y, stats, scale_shift, batch_stats = bn_relu_rows_forward(z, gamma, beta, eps, residual=r)
        ctx.save_for_backward(gamma, stats, scale_shift, z, r)
        ctx.mark_non_differentiable(batch_stats)
        return y, batch_stats

    @staticmethod
    def backward(ctx, grad_y, _grad_stats):
        gamma, stats, scale_shift, z, r = ctx.saved_tensors
        dz, dr, d_gamma, d_beta = bn_relu_rows_backward(z, grad_y, gamma, stats, scale_shift, residual=r)
        need = ctx.needs_input_grad
        return (None, d_gamma if need[1] else None, d_beta if need[2] else None, dz if need[3] else None,
                dr if need[4] else None)


def bn_relu_train(z, bn, residual=None):
    """relu(bn(z)) or relu(bn(z) + residual) for a train-mode BatchNorm1d module `bn` on an (N, C) fp32 feature matrix, differentiable
    with respect to z, the residual and the module's weight / bias; running_mean / running_var / num_batches_tracked are updated
    in place as BatchNorm1d does (momentum form, unbiased variance), exactly as bev_train.bn_relu_train does for BatchNorm2d.
    Needs bn_supported(bn, C) and N >= 2.  No host synchronisation."""
    if z.dim() != 2 or not bn_supported(bn, z.shape[1]):
        raise _lib.LidarHipError(f"spconv.bn_relu_train: unsupported BatchNorm1d / feature matrix {tuple(z.shape)} (bn_supported)")
    z = z.contiguous()
    if residual is None:
        y, batch_stats = _BNReLURows.apply(float(bn.eps), bn.weight, bn.bias, z)
    else:
        y, batch_stats = _BNAddReLURows.apply(float(bn.eps), bn.weight, bn.bias, z, residual.contiguous())
    c, m = bn.num_features, float(bn.momentum)
    with torch.no_grad():   # BatchNorm1d's running update (momentum form), on the device
        bn.running_mean.mul_(1.0 - m).add_(batch_stats[:c], alpha=m)
        bn.running_var.mul_(1.0 - m).add_(batch_stats[2 * c:3 * c], alpha=m)
        bn.num_batches_tracked.add_(1)
    return y
