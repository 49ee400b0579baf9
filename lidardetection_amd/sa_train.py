"""Train-mode set abstraction on this package's kernels (csrc/sa_train.hip).

reference: pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py:58-92 (StackSAModuleMSG.forward), pointnet2_utils.py:104-160
(QueryAndGroup) and src/group_points_gpu.cu:15-45 (the grouping gradient: one float atomicAdd per element).

A scale of StackSAModuleMSG in grad mode, row-major: the first 1x1 convolution runs per SOURCE point in front of the gather
(torch.mm, so autograd yields its weight and feature gradients), `sa_gather_train` gathers its rows per (query, sample) pair and
sends the gradient back through an inverse index (ordered sums, no float atomics), the middle layers are torch.mm plus the fused
row BatchNorm + ReLU of bn_train.py, and `bn_relu_max_train` is the last layer's BatchNorm + ReLU + max over the samples in
one pass that never writes the (M * nsample, H) activation.

Opt-in: inside `with fused_sa_train():` a grad-mode, train-mode StackSAModuleMSG whose scales all qualify (scale_supported) takes
this route; outside it nothing changes.
"""
import torch
from torch import nn

from . import _lib, bn_train

MAX_H, MAX_NSAMPLE = 128, 64          # csrc/sa_train.hip SAT_MAX_H / SAT_MAX_NS

fused_sa_train, fused_sa_train_enabled = bn_train.switch(
    """inside: a grad-mode, train-mode StackSAModuleMSG with pool_method 'max_pool' runs on the fused route when every one of its
    scales qualifies (module_supported); anything else, and everything outside, runs the stock modules""")


def supported(H, nsample):
    """the kernels take this width and sample count: H % 4 == 0, 4 <= H <= 128, 1 <= nsample <= 64.  Pure host."""
    return bool(_lib.lib().lidar_sa_train_supported(int(H), int(nsample)))


def _bn_ok(bn):
    return bn_train.supported(bn, nn.BatchNorm2d, True, max_c=None)     # the width is supported()'s business


def scale_supported(mlp, nsample):
    """a scale's shared MLP qualifies: Conv2d(1x1, bias=False) -> BatchNorm2d -> ReLU two or more times, every width inside the
    kernels' support, every BatchNorm affine and tracking running statistics with a numeric momentum.  Pure host."""
    mods = list(mlp)
    if len(mods) % 3 or len(mods) < 6:
        return False
    for conv, bn, act in zip(mods[0::3], mods[1::3], mods[2::3]):
        if not (isinstance(conv, nn.Conv2d) and conv.bias is None and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
                and conv.groups == 1 and isinstance(act, nn.ReLU) and _bn_ok(bn) and bn.num_features == conv.out_channels
                and supported(conv.out_channels, nsample)):
            return False
    return True


def module_supported(module):
    """every scale of this StackSAModuleMSG qualifies for the fused route (and it pools by maximum, in train mode).  Pure host."""
    return (module.training and module.pool_method == 'max_pool'
            and all(scale_supported(mlp, g.nsample) for mlp, g in zip(module.mlps, module.groupers)))


def _f32(what, t, shape=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) or (shape is not None and tuple(t.shape) != tuple(shape)):
        _lib.fail(what, f"expected a contiguous float32 CUDA (ROCm) tensor{'' if shape is None else ' of shape ' + str(tuple(shape))}, "
                        f"got {t.dtype} {tuple(t.shape)} on {t.device}")


def _sizes(what, H, nsample, M):
    if not supported(H, nsample) or M * nsample >= 2 ** 31:
        _lib.fail(what, f"needs H % 4 == 0, 4 <= H <= {MAX_H}, 1 <= nsample <= {MAX_NSAMPLE} and M * nsample < 2^31, got H {H}, "
                        f"nsample {nsample}, M {M}")


# ---- (a) - (c): the gather -------------------------------------------------------------------------------------------------------
def sa_gather_forward(table, query_term, idx, xyz_batch_cnt, new_xyz_batch_cnt):
    """table (N, H), query_term (M, H) or None, idx (M, nsample) raw ball-query result -> z (M * nsample, H)"""
    M, ns = idx.shape
    N, H = table.shape
    _sizes("sa_gather_forward", H, ns, M)
    _f32("sa_gather_forward", table)
    if query_term is not None:
        _f32("sa_gather_forward", query_term, (M, H))
    _lib.require_cuda(idx, xyz_batch_cnt, new_xyz_batch_cnt)
    z = torch.empty((M * ns, H), dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().lidar_sa_gather_train_forward(xyz_batch_cnt.shape[0], M, N, H, ns, _lib.ptr(table), _lib.ptr(query_term),
                                                        _lib.ptr(xyz_batch_cnt), _lib.ptr(idx), _lib.ptr(new_xyz_batch_cnt),
                                                        _lib.ptr(z), _lib.stream()), "lidar_sa_gather_train_forward")
    return z


def inverse_index(idx, xyz_batch_cnt, new_xyz_batch_cnt, N):
    """-> (row_start (N + 1), pairs (M * nsample)) int32: source row n is read by the pairs pairs[row_start[n]:row_start[n + 1]], in
    ascending pair number m * nsample + s; the pairs of empty balls follow from row_start[N] on.  The keys are a kernel, the
    ordering a stable torch.sort of them, row_start a kernel on the sorted keys.  No host synchronisation."""
    M, ns = idx.shape
    _lib.require_cuda(idx, xyz_batch_cnt, new_xyz_batch_cnt)
    if not 1 <= ns <= MAX_NSAMPLE or M * ns >= 2 ** 31:
        _lib.fail("inverse_index", f"needs 1 <= nsample <= {MAX_NSAMPLE} and M * nsample < 2^31, got {tuple(idx.shape)}")
    dev, L = idx.device, _lib.lib()
    keys = torch.empty(M * ns, dtype=torch.int32, device=dev)
    _lib.check(L.lidar_sa_pair_keys(xyz_batch_cnt.shape[0], M, int(N), ns, _lib.ptr(xyz_batch_cnt), _lib.ptr(idx),
                                    _lib.ptr(new_xyz_batch_cnt), _lib.ptr(keys), _lib.stream()), "lidar_sa_pair_keys")
    sorted_keys, order = torch.sort(keys, stable=True)
    pairs = order.to(torch.int32)
    row_start = torch.empty(int(N) + 1, dtype=torch.int32, device=dev)
    _lib.check(L.lidar_sa_row_start(M * ns, int(N), _lib.ptr(sorted_keys), _lib.ptr(row_start), _lib.stream()), "lidar_sa_row_start")
    return row_start, pairs


def sa_gather_backward(dz, idx, row_start, pairs, N, need_query=True):
    """dz (M * nsample, H) -> (d_table (N, H), d_query (M, H) or None)"""
    M, ns = idx.shape
    H = dz.shape[1]
    _sizes("sa_gather_backward", H, ns, M)
    _f32("sa_gather_backward", dz, (M * ns, H))
    _lib.require_cuda(idx, row_start, pairs)
    if row_start.numel() != N + 1 or pairs.numel() != M * ns:
        _lib.fail("sa_gather_backward", f"row_start must hold {N + 1} and pairs {M * ns} entries")
    d_table = torch.empty((N, H), dtype=torch.float32, device=dz.device)
    d_query = torch.empty((M, H), dtype=torch.float32, device=dz.device) if need_query else None
    _lib.check(_lib.lib().lidar_sa_gather_train_backward(M, N, H, ns, _lib.ptr(dz), _lib.ptr(idx), _lib.ptr(row_start), _lib.ptr(pairs),
                                                         _lib.ptr(d_table), _lib.ptr(d_query), _lib.stream()),
               "lidar_sa_gather_train_backward")
    return d_table, d_query


class _SAGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, query_term, idx, xyz_batch_cnt, new_xyz_batch_cnt):
        ctx.save_for_backward(idx, xyz_batch_cnt, new_xyz_batch_cnt)
        ctx.n_src = table.shape[0]
        return sa_gather_forward(table, query_term, idx, xyz_batch_cnt, new_xyz_batch_cnt)

    @staticmethod
    def backward(ctx, dz):
        idx, xyz_cnt, new_cnt = ctx.saved_tensors
        N = ctx.n_src
        need = ctx.needs_input_grad
        row_start, pairs = inverse_index(idx, xyz_cnt, new_cnt, N)
        d_table, d_query = sa_gather_backward(dz.contiguous(), idx, row_start, pairs, N, need_query=need[1])
        return d_table if need[0] else None, d_query, None, None, None


def sa_gather_train(table, query_term, idx, xyz_batch_cnt, new_xyz_batch_cnt):
    """z (M * nsample, H): row (m, s) = table[start_b + idx[m][s]] - query_term[m], exactly 0 for an empty ball; differentiable with
    respect to table and query_term (None: no query term).  idx is the raw ball-query result (idx[m][0] < 0: empty ball)."""
    return _SAGather.apply(table.contiguous(), None if query_term is None else query_term.contiguous(), idx, xyz_batch_cnt,
                           new_xyz_batch_cnt)


# ---- (d): BatchNorm + ReLU + max ---------------------------------------------------------------------------------------------------
def bn_relu_max_forward(z, M, nsample, gamma, beta, eps):
    """z (M * nsample, H) -> (out (M, H), arg (M, H) uint8, stats, scale_shift, batch_stats)"""
    H = z.shape[1] if z.dim() == 2 else -1
    _sizes("bn_relu_max_forward", H, nsample, M)
    _f32("bn_relu_max_forward", z, (M * nsample, H))
    _lib.require_cuda(gamma, beta)
    if M * nsample < 2 or gamma.numel() != H or beta.numel() != H:
        _lib.fail("bn_relu_max_forward", f"needs at least 2 rows and {H} gamma / beta values")
    dev = z.device
    out = torch.empty((M, H), dtype=torch.float32, device=dev)
    arg = torch.empty((M, H), dtype=torch.uint8, device=dev)
    stats, scale_shift, batch_stats = bn_train.alloc_stats(H, dev)
    ws, wsb = bn_train.get_workspace("sa_train", dev, M, nsample, H)
    _lib.check(_lib.lib().lidar_bn_relu_max_train_forward(_lib.ptr(z), M, nsample, H, _lib.ptr(gamma), _lib.ptr(beta), float(eps),
                                                          _lib.ptr(out), _lib.ptr(arg), _lib.ptr(stats), _lib.ptr(scale_shift),
                                                          _lib.ptr(batch_stats), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_relu_max_train_forward")
    return out, arg, stats, scale_shift, batch_stats


def bn_relu_max_backward(z, M, nsample, grad_out, arg, gamma, stats, scale_shift):
    """-> (dz (M * nsample, H), d_gamma, d_beta)"""
    H = z.shape[1] if z.dim() == 2 else -1
    _sizes("bn_relu_max_backward", H, nsample, M)
    _f32("bn_relu_max_backward", z, (M * nsample, H))
    g = grad_out.contiguous()
    _f32("bn_relu_max_backward", g, (M, H))
    if M * nsample < 2 or not (arg.is_cuda and arg.dtype == torch.uint8 and arg.is_contiguous() and tuple(arg.shape) == (M, H)):
        _lib.fail("bn_relu_max_backward", f"needs at least 2 rows and a contiguous uint8 CUDA arg of shape {(M, H)}")
    _lib.require_cuda(gamma, scale_shift)
    dev = z.device
    dz = torch.empty_like(z)
    d_gamma = torch.empty(H, dtype=torch.float32, device=dev)
    d_beta = torch.empty(H, dtype=torch.float32, device=dev)
    ws, wsb = bn_train.get_workspace("sa_train", dev, M, nsample, H)
    _lib.check(_lib.lib().lidar_bn_relu_max_train_backward(_lib.ptr(z), M, nsample, H, _lib.ptr(g), _lib.ptr(arg), _lib.ptr(gamma),
                                                           _lib.ptr(stats), _lib.ptr(scale_shift), _lib.ptr(dz), _lib.ptr(d_gamma),
                                                           _lib.ptr(d_beta), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_relu_max_train_backward")
    return dz, d_gamma, d_beta


class _BNReLUMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eps, gamma, beta, z, M, nsample):
        out, arg, stats, scale_shift, batch_stats = bn_relu_max_forward(z, M, nsample, gamma, beta, eps)
        ctx.save_for_backward(gamma, stats, scale_shift, z, arg)       # z and arg only: y and the ReLU mask are recomputed
        ctx.sizes = (M, nsample)
        ctx.mark_non_differentiable(batch_stats)
        return out, batch_stats

    @staticmethod
    def backward(ctx, grad_out, _grad_stats):
        gamma, stats, scale_shift, z, arg = ctx.saved_tensors
        dz, d_gamma, d_beta = bn_relu_max_backward(z, *ctx.sizes, grad_out, arg, gamma, stats, scale_shift)
        need = ctx.needs_input_grad
        return None, d_gamma if need[1] else None, d_beta if need[2] else None, dz if need[3] else None, None, None


def bn_relu_max_train(z, bn, M, nsample):
    """max over the nsample rows of every query of relu(bn(z)) for a train-mode BatchNorm2d module `bn` on the (M * nsample, H)
    matrix z -> (M, H); differentiable with respect to z and the module's weight / bias.  running_mean / running_var /
    num_batches_tracked are updated in place as bev_train.bn_relu_train does for BatchNorm2d.  No host synchronisation."""
    if not _bn_ok(bn) or z.dim() != 2 or bn.num_features != z.shape[1]:
        _lib.fail("bn_relu_max_train", f"unsupported BatchNorm2d / matrix {tuple(z.shape)}")
    out, batch_stats = _BNReLUMax.apply(float(bn.eps), bn.weight, bn.bias, z.contiguous(), int(M), int(nsample))
    bn_train.update_module(bn, batch_stats)
    return out


def bn_relu_rows_train(z, bn):
    """relu(bn(z)) on the (rows, H) matrix z for a train-mode BatchNorm2d module (a middle layer): bn_train.py's rows path"""
    y, batch_stats = bn_train._BNReLURows.apply(float(bn.eps), bn.weight, bn.bias, z.contiguous())
    bn_train.update_module(bn, batch_stats)
    return y


# ---- one scale -----------------------------------------------------------------------------------------------------------------------
def scale_forward(mlp, nsample, use_xyz, xyz, new_xyz, features, idx, xyz_batch_cnt, new_xyz_batch_cnt):
    """One qualifying scale (scale_supported) of StackSAModuleMSG in train mode -> (M, H_last).  idx: the raw ball-query result."""
    mods = list(mlp)
    convs, bns = mods[0::3], mods[1::3]
    M = new_xyz.shape[0]
    w1 = convs[0].weight[:, :, 0, 0]                                   # (H1, [3 +] C)
    if use_xyz:
        src = xyz if features is None else torch.cat((xyz, features), dim=1)
        table = torch.mm(src, w1.t())
        query_term = torch.mm(new_xyz, w1[:, :3].t())
    else:
        table, query_term = torch.mm(features, w1.t()), None
    z = sa_gather_train(table, query_term, idx, xyz_batch_cnt, new_xyz_batch_cnt)
    for conv, bn in zip(convs[1:], bns[:-1]):
        z = torch.mm(bn_relu_rows_train(z, bn), conv.weight[:, :, 0, 0].t())
    return bn_relu_max_train(z, bns[-1], M, nsample)
