"""What every fused train-mode BatchNorm + ReLU route shares on the host: the predicate "the kernels take this module",
the result buffers, the workspace, the running-statistics update, the opt-in switch, and the (N, C) rows path of csrc/bn_train.hip
with its autograd functions.  bev_train (dense maps), spconv.train (sparse features), sa_train (set abstraction) and
pillar_ops.pillar_vfe_train are the callers; a new route starts here.
"""
import contextlib
import ctypes as C

import torch
from torch import nn

from . import _lib, workspace

MAX_C = 1024          # channels of one input (csrc/bn_train_dev.h BT_MAX_C)
_WS_BYTES = {"bn_train": "lidar_bn_relu_train_workspace_bytes", "sa_train": "lidar_bn_relu_max_train_workspace_bytes"}


def supported(bn, cls, require_training, channels=None, max_c=MAX_C):
    """the fused kernels take module `bn`: an instance of `cls` (in training mode when require_training), affine, with running
    statistics and a numeric momentum (momentum=None's cumulative average stays on torch), `channels` (default: its own width) equal
    to num_features, a multiple of 4 in [4, max_c] (max_c=None: the caller checks the width itself).  Pure host."""
    if not isinstance(bn, cls) or (require_training and not bn.training):
        return False
    c = bn.num_features if channels is None else int(channels)
    return bool(bn.affine and bn.track_running_stats and bn.running_mean is not None and bn.num_batches_tracked is not None
                and isinstance(bn.momentum, (int, float)) and not isinstance(bn.momentum, bool) and c == bn.num_features
                and (max_c is None or (c % 4 == 0 and 4 <= c <= max_c)))


def switch(doc):
    """-> (a context manager `scope(enabled=True)` with docstring `doc`, a function telling whether a scope is open): the opt-in
    switch of one fused route, off outside every scope"""
    state = [False]

    @contextlib.contextmanager
    def scope(enabled=True):
        was = state[0]
        state[0] = bool(enabled)
        try:
            yield
        finally:
            state[0] = was

    scope.__doc__ = doc
    return scope, lambda: state[0]


def alloc_stats(ctot, device):
    """-> (stats (2 ctot,) fp64: mean | 1 / sigma, scale_shift (2 ctot,) fp32, batch_stats (3 ctot,) fp32: mean | biased variance |
    unbiased variance), uninitialised, for the forward entry points to fill"""
    return (torch.empty(2 * ctot, dtype=torch.float64, device=device), torch.empty(2 * ctot, dtype=torch.float32, device=device),
            torch.empty(3 * ctot, dtype=torch.float32, device=device))


def get_workspace(name, device, *sizes):
    """-> (ws, its byte count) for workspace `name` ("bn_train": sizes = rows, channels; "sa_train": M, nsample, H), the byte count
    asked of the library"""
    wsb = getattr(_lib.lib(), _WS_BYTES[name])(*sizes)
    return workspace.get(name, wsb, device), wsb


def update_running(running_mean, running_var, num_batches_tracked, momentum, batch_stats, c, ctot=None, off=0):
    """BatchNorm's running update (momentum form, unbiased variance) with torch ops on the device-computed batch_stats of a fused
    call over ctot channels (default c), for the module that owns channels [off, off + c): the tensors' version counters move as
    BatchNorm's own update moves them.  num_batches_tracked may be None."""
    ctot = c if ctot is None else ctot
    with torch.no_grad():
        running_mean.mul_(1.0 - momentum).add_(batch_stats[off:off + c], alpha=momentum)
        running_var.mul_(1.0 - momentum).add_(batch_stats[2 * ctot + off:2 * ctot + off + c], alpha=momentum)
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)


def update_module(bn, batch_stats, ctot=None, off=0):
    """update_running for a BatchNorm module"""
    update_running(bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), batch_stats, bn.num_features, ctot, off)


# ------------------------------------------------------------------ the rows path: an (N, C) matrix, one segment, row stride C
def _check_rows(what, z, r=None):
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.is_contiguous()):
        raise _lib.LidarHipError(f"{what}: expected a contiguous 2-d float32 CUDA (ROCm) matrix, got {z.dtype} {tuple(z.shape)} on {z.device}")
    n, c = z.shape
    if n < 2 or c % 4 or not 4 <= c <= MAX_C:
        raise _lib.LidarHipError(f"{what}: needs at least 2 rows and a multiple of 4 channels in [4, {MAX_C}], got {tuple(z.shape)}")
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
    y = torch.empty_like(z)
    stats, scale_shift, batch_stats = alloc_stats(c, z.device)
    ws, wsb = get_workspace("bn_train", z.device, n, c)
    L = _lib.lib()
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
    ws, wsb = get_workspace("bn_train", dev, n, c)
    L = _lib.lib()
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
    """apply(eps, gamma, beta, z): relu(bn(z)) -> (y, batch_stats); with a fifth argument r, relu(bn(z) + r) (_BNAddReLURows)"""

    @staticmethod
    def forward(ctx, eps, gamma, beta, z, r=None):
        y, stats, scale_shift, batch_stats = bn_relu_rows_forward(z, gamma, beta, eps, residual=r)
        ctx.save_for_backward(gamma, stats, scale_shift, z, *([] if r is None else [r]))    # z (and r) only: y and the ReLU mask are recomputed
        ctx.mark_non_differentiable(batch_stats)
        return y, batch_stats

    @staticmethod
    def backward(ctx, grad_y, _grad_stats):
        gamma, stats, scale_shift, z, *r = ctx.saved_tensors
        dz, dr, d_gamma, d_beta = bn_relu_rows_backward(z, grad_y, gamma, stats, scale_shift, residual=r[0] if r else None)
        need = ctx.needs_input_grad
        grads = (None, d_gamma if need[1] else None, d_beta if need[2] else None, dz if need[3] else None)
        return grads + ((dr if need[4] else None,) if r else ())


class _BNAddReLURows(_BNReLURows):
    """the residual form: the same body under the name its graph nodes carry"""


def bn_relu_rows_train(z, bn, residual=None):
    """relu(bn(z)) or relu(bn(z) + residual) for a train-mode BatchNorm1d module `bn` on an (N, C) fp32 feature matrix, differentiable
    with respect to z, the residual and the module's weight / bias; running_mean / running_var / num_batches_tracked are updated
    in place as BatchNorm1d does (momentum form, unbiased variance), exactly as bev_train.bn_relu_train does for BatchNorm2d.
    Needs supported(bn, BatchNorm1d, training, C) and N >= 2.  No host synchronisation.  (spconv.train.bn_relu_train)"""
    if z.dim() != 2 or not supported(bn, nn.BatchNorm1d, True, z.shape[1]):
        raise _lib.LidarHipError(f"spconv.bn_relu_train: unsupported BatchNorm1d / feature matrix {tuple(z.shape)} (bn_supported)")
    z = z.contiguous()
    if residual is None:
        y, batch_stats = _BNReLURows.apply(float(bn.eps), bn.weight, bn.bias, z)
    else:
        y, batch_stats = _BNAddReLURows.apply(float(bn.eps), bn.weight, bn.bias, z, residual.contiguous())
    update_module(bn, batch_stats)
    return y
