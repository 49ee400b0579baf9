"""Train-mode BatchNorm1d + ReLU on sparse features, fused (csrc/bn_train.hip).

reference: pcdet/models/backbones_3d/spconv_backbone.py:7-26 (post_act_block: conv -> BatchNorm1d -> ReLU) and :29-65
(SparseBasicBlock: bn1 -> relu, bn2 -> += identity -> relu).

The features of a SparseConvTensor are an (N, C) matrix, which is the `rows x C` map the dense backbone's fused train-mode
BatchNorm + ReLU kernels take with one segment, rows = N and row stride C: fp64 fixed-order batch statistics, y = relu(bn(z)) in one
pass, the backward's ReLU mask recomputed from z (only z is saved), no float atomics and no host read.  The residual form
y = relu(bn(z) + r) is the same kernels with the residual added before the ReLU (lidar_bn_add_relu_train_*).  The rows path itself
(bn_relu_rows_forward / _backward, the autograd functions, the running-statistics update) lives in ../bn_train.py, shared with the
set abstraction's middle layers; this module is the sparse backbone's face of it.

Opt-in: inside `with fused_bn_train():` a grad-mode SparseSequential runs every supported BatchNorm1d -> ReLU pair as the fused
call and SparseBasicBlock runs bn1 -> relu and bn2 -> += identity -> relu on them; outside it nothing changes.
"""
import torch
from torch import nn

from .. import bn_train as _shared
from ..bn_train import bn_relu_rows_backward, bn_relu_rows_forward  # noqa: F401  (re-exported)

fused_bn_train, fused_bn_train_enabled = _shared.switch(
    """inside: grad-mode SparseSequential / SparseBasicBlock run their train-mode BatchNorm1d (+ residual) + ReLU on the fused kernels
    wherever bn_supported() holds and the tensor has at least 2 rows; anything else runs the modules as outside""")


def bn_supported(bn, channels=None):
    """the fused kernels take this BatchNorm1d: in training mode, affine, tracking running statistics with a numeric momentum
    (momentum=None's cumulative average stays on torch), C % 4 == 0 and 4 <= C <= 1024.  Pure host."""
    return _shared.supported(bn, nn.BatchNorm1d, True, channels)


def takes(bn, feats):
    """the fused route applies to module `bn` on the feature matrix `feats` (bn_supported, fp32 on the device, N >= 2)"""
    return (bn_supported(bn, feats.shape[1] if feats.dim() == 2 else -1) and feats.is_cuda and feats.dtype == torch.float32
            and feats.shape[0] >= 2 and bn.weight.is_cuda and bn.weight.dtype == torch.float32)


def bn_relu_train(z, bn, residual=None):
    """relu(bn(z)) or relu(bn(z) + residual) for a train-mode BatchNorm1d module `bn` on an (N, C) fp32 feature matrix, differentiable
    with respect to z, the residual and the module's weight / bias; running_mean / running_var / num_batches_tracked are updated
    in place as BatchNorm1d does (bn_train.bn_relu_rows_train).  Needs bn_supported(bn, C) and N >= 2.  No host synchronisation."""
    return _shared.bn_relu_rows_train(z, bn, residual)
