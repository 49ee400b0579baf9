"""Host side of the PillarVFE / MeanVFE / PointPillarScatter kernels (include/lidar_hip.h)."""
import torch

from . import _lib, bn_train, workspace
from ._lib import LIMITS


def fold_bn(gamma, beta, mean, var, eps):
    """BatchNorm1d (eval) -> per-channel scale/shift: y = x*scale + shift."""
    scale = gamma / torch.sqrt(var + eps)
    return scale.contiguous(), (beta - mean * scale).contiguous()


def pillar_vfe(voxels, num_points, coords, weight, scale, shift, voxel_size, point_cloud_range,
               with_distance=False, num_voxels_dev=None):
    """Fused PillarVFE (single PFN layer, eval).  voxels (V,P,C) f32; num_points (V) i32|f32;
    coords (V,4) [b,z,y,x] i32|f32; weight (cout, C+6[+1]); -> (V, cout) f32.
    Reference: pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-123 + PFNLayer :29-49."""
    _lib.require_cuda(voxels, num_points, coords, weight, scale, shift)
    V, P, C = voxels.shape
    cout = weight.shape[0]
    if weight.shape[1] != C + 6 + int(bool(with_distance)):
        raise _lib.LidarHipError("weight must be (cout, C + 6 [+1 with_distance]) — use_absolute_xyz layout")
    if coords.dtype not in (torch.int32, torch.float32) or num_points.dtype not in (torch.int32, torch.float32):
        raise _lib.LidarHipError("coords / num_points must be int32 or float32")
    out = torch.empty((V, cout), dtype=torch.float32, device=voxels.device)
    L = _lib.lib()
    _lib.check(L.lidar_pillar_vfe(_lib.ptr(voxels), _lib.ptr(num_points), _lib.ptr(coords), V, _lib.ptr(num_voxels_dev),
                                  P, C, _lib.ptr(weight), _lib.ptr(scale), _lib.ptr(shift), cout,
                                  _lib.host_f32(voxel_size), _lib.host_f32(point_cloud_range), int(bool(with_distance)),
                                  int(coords.dtype == torch.float32), int(num_points.dtype == torch.float32),
                                  _lib.ptr(out), _lib.stream()), "lidar_pillar_vfe")
    return out


def mean_vfe(voxels, num_points):
    """MeanVFE (pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31) -> (V, C)."""
    _lib.require_cuda(voxels, num_points)
    V, P, C = voxels.shape
    out = torch.empty((V, C), dtype=torch.float32, device=voxels.device)
    L = _lib.lib()
    _lib.check(L.lidar_mean_vfe(_lib.ptr(voxels), _lib.ptr(num_points), V, P, C, int(num_points.dtype == torch.float32),
                                _lib.ptr(out), _lib.stream()), "lidar_mean_vfe")
    return out


def pillar_scatter(pillar_features, coords, batch_size, nx, ny, num_voxels_dev=None, out=None, channels_last=False):
    """PointPillarScatter (pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:14-37), nz == 1.
    pillar_features (V, C) f32, coords (V,4) [b,z,y,x] i32|f32 -> (B, C, ny, nx) f32."""
    _lib.require_cuda(pillar_features, coords)
    V, C = pillar_features.shape
    if out is None:
        out = torch.empty((batch_size, C, ny, nx), dtype=torch.float32, device=pillar_features.device,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    L = _lib.lib()
    wsb = L.lidar_pillar_scatter_workspace_bytes(batch_size, nx, ny)
    ws = workspace.get("scatter", wsb, pillar_features.device)
    _lib.check(L.lidar_pillar_scatter(_lib.ptr(pillar_features), _lib.ptr(coords), int(coords.dtype == torch.float32), V,
                                      _lib.ptr(num_voxels_dev), C, batch_size, nx, ny, int(bool(channels_last)), _lib.ptr(out),
                                      _lib.ptr(ws), wsb,
                                      _lib.stream()), "lidar_pillar_scatter")
    return out


class ResidentCanvas:
    """One persistent channels-last BEV canvas (B, C, ny, nx) kept in HBM across calls: update() clears the cells the previous
    call wrote and writes the new pillars (~2*V*C*4 bytes instead of rewriting the > 90 % zero canvas).  After update() the
    canvas equals pillar_scatter(..., channels_last=True) of the same pillars."""

    def __init__(self, batch_size, channels, ny, nx, max_pillars, device):
        self.B, self.C, self.ny, self.nx, self.cap = batch_size, channels, ny, nx, int(max_pillars)
        self.canvas = torch.zeros((batch_size, channels, ny, nx), dtype=torch.float32, device=device).contiguous(
            memory_format=torch.channels_last)
        self.prev_cells = torch.full((max(self.cap, 1),), -1, dtype=torch.int32, device=device)
        self.prev_count = torch.zeros((1,), dtype=torch.int32, device=device)

    def update(self, pillar_features, coords, num_voxels_dev=None):
        _lib.require_cuda(pillar_features, coords)
        V, C = pillar_features.shape
        if C != self.C or V > self.cap:
            raise _lib.LidarHipError("ResidentCanvas.update: feature width / pillar count exceeds what the canvas was built for")
        _lib.check(_lib.lib().lidar_pillar_scatter_update(_lib.ptr(pillar_features), _lib.ptr(coords), int(coords.dtype == torch.float32), V,
                                                          _lib.ptr(num_voxels_dev), C, self.B, self.nx, self.ny, _lib.ptr(self.canvas),
                                                          _lib.ptr(self.prev_cells), _lib.ptr(self.prev_count), _lib.stream()),
                   "lidar_pillar_scatter_update")
        return self.canvas


def pillar_conv_table(coords, batch_size, nx, ny, k, stride, pad, num_voxels_dev=None):
    """Neighbour table of the k x k / stride / pad convolution that follows PointPillarScatter, over all output pixels in NHWC map
    order: (B * OH * OW, k * k) int32 pillar rows or -1 (csrc/pillar.hip lidar_pillar_conv_table).  -> (nbr, OH, OW)"""
    _lib.require_cuda(coords)
    if coords.dtype not in (torch.int32, torch.float32) or coords.dim() != 2 or coords.shape[1] != 4:
        raise _lib.LidarHipError("pillar_conv_table: coords must be (V, 4) [b, z, y, x] int32 or float32")
    OH, OW = (ny + 2 * pad - k) // stride + 1, (nx + 2 * pad - k) // stride + 1
    L = _lib.lib()
    nbr = torch.empty((batch_size * OH * OW, k * k), dtype=torch.int32, device=coords.device)
    wsb = L.lidar_pillar_conv_table_workspace_bytes(batch_size, nx, ny)
    ws = workspace.get("pillar_conv_table", wsb, coords.device)
    _lib.check(L.lidar_pillar_conv_table(_lib.ptr(coords), int(coords.dtype == torch.float32), coords.shape[0], _lib.ptr(num_voxels_dev),
                                         batch_size, nx, ny, int(k), int(stride), int(pad), _lib.ptr(nbr), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_pillar_conv_table")
    return nbr, OH, OW


class PillarMap:
    """What PointPillarScatter's output IS before anybody materialises it: the PFN rows, their coordinates and the count (on the
    device).  A consumer that can work from the pillars (FoldedBEVBackbone's sparse first layer) never builds the > 90 %-zero
    canvas; dense() gives the ordinary channels-last canvas (through the owner's ResidentCanvas) to everybody else."""

    def __init__(self, features, coords, num_voxels_dev, batch_size, nx, ny, dense_fn):
        self.features, self.coords, self.num_voxels_dev = features, coords, num_voxels_dev
        self.B, self.nx, self.ny, self._dense_fn = batch_size, nx, ny, dense_fn

    def dense(self):
        return self._dense_fn(self.features, self.coords, self.num_voxels_dev)


# ------------------------------------------------------------------ training (csrc/pfn_train.hip)
_STATS_DOUBLES = LIMITS["LIDAR_PFN_TRAIN_STATS_DOUBLES"]      # lidar_pfn_train_forward's `stats`


def pfn_train_supported(num_features, max_points, cout):
    """the configurations the fused train-mode PFN covers (the eval kernel's range); everything else stays on torch"""
    return 3 <= int(num_features) <= 8 and 0 < int(max_points) <= 64 and 0 < int(cout) <= 64


class _PillarVFETrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, voxels, num_points, coords, num_voxels_dev, weight, gamma, beta):
        V, P, C = voxels.shape
        cout = weight.shape[0]
        dev = voxels.device
        out = torch.empty((V, cout), dtype=torch.float32, device=dev)
        zsel = torch.empty((V, cout), dtype=torch.float32, device=dev)
        slot = torch.empty((V, cout), dtype=torch.uint8, device=dev)
        stats = torch.empty(_STATS_DOUBLES, dtype=torch.float64, device=dev)
        scale_shift = torch.empty(2 * cout, dtype=torch.float32, device=dev)
        batch_stats = torch.empty(3 * cout, dtype=torch.float32, device=dev)
        L = _lib.lib()
        wsb = L.lidar_pfn_train_workspace_bytes(V, C, cout, meta["dist"])
        ws = workspace.get("pfn_train", wsb, dev)
        _lib.check(L.lidar_pfn_train_forward(_lib.ptr(voxels), _lib.ptr(num_points), _lib.ptr(coords), V, _lib.ptr(num_voxels_dev), P, C,
                                             _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta), cout, meta["eps"], meta["vs"], meta["rng"],
                                             meta["dist"], meta["cf"], meta["nf"], _lib.ptr(out), _lib.ptr(zsel), _lib.ptr(slot),
                                             _lib.ptr(stats), _lib.ptr(scale_shift), _lib.ptr(batch_stats), _lib.ptr(ws), wsb,
                                             _lib.stream()), "lidar_pfn_train_forward")
        ctx.meta = meta
        ctx.save_for_backward(voxels, num_points, coords, num_voxels_dev, weight, gamma, zsel, slot, stats, scale_shift)
        ctx.mark_non_differentiable(batch_stats)
        return out, batch_stats

    @staticmethod
    def backward(ctx, grad_out, _grad_stats):
        meta = ctx.meta
        voxels, num_points, coords, nvd, weight, gamma, zsel, slot, stats, scale_shift = ctx.saved_tensors
        V, P, C = voxels.shape
        cout = weight.shape[0]
        g = grad_out.contiguous()
        d_w, d_g, d_b = torch.empty_like(weight), torch.empty_like(gamma), torch.empty_like(gamma)
        L = _lib.lib()
        wsb = L.lidar_pfn_train_workspace_bytes(V, C, cout, meta["dist"])
        ws = workspace.get("pfn_train", wsb, voxels.device)
        _lib.check(L.lidar_pfn_train_backward(_lib.ptr(voxels), _lib.ptr(num_points), _lib.ptr(coords), V, _lib.ptr(nvd), P, C,
                                              _lib.ptr(weight), _lib.ptr(gamma), cout, meta["vs"], meta["rng"], meta["dist"], meta["cf"],
                                              meta["nf"], _lib.ptr(g), _lib.ptr(zsel), _lib.ptr(slot), _lib.ptr(stats),
                                              _lib.ptr(scale_shift), _lib.ptr(d_w), _lib.ptr(d_g), _lib.ptr(d_b), _lib.ptr(ws), wsb,
                                              _lib.stream()), "lidar_pfn_train_backward")
        need = ctx.needs_input_grad
        return (None, None, None, None, None, d_w if need[5] else None, d_g if need[6] else None, d_b if need[7] else None)


def pillar_vfe_train(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, voxel_size, point_cloud_range,
                     with_distance=False, eps=1e-3, momentum=0.01, num_batches_tracked=None, num_voxels_dev=None, return_stats=False):
    """PillarVFE with one PFNLayer (USE_NORM, USE_ABSLOTE_XYZ) in TRAIN mode, differentiable with respect to weight (cout, C + 6 [+1]),
    gamma and beta (the BatchNorm1d's weight and bias); pillar_vfe.py:29-49, :94-123.  The batch statistics run over all
    num_voxels * P rows (padded slots included), num_voxels = num_voxels_dev (a device int, rows past it are neither read nor counted)
    or V.  running_mean / running_var (and num_batches_tracked) are updated in place as BatchNorm1d does, with torch ops on the
    device-computed batch statistics (their version counters move).  No host synchronisation.  -> pillar_features (V, cout);
    rows past the device count are zero.  The voxels get no gradient.  return_stats: -> (pillar_features, batch mean, biased batch
    variance), the statistics as (cout,) device tensors."""
    _lib.require_cuda(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, num_voxels_dev)
    if voxels.dim() != 3:
        raise _lib.LidarHipError("pillar_vfe_train: voxels must be (V, P, C)")
    V, P, C = voxels.shape
    cout = weight.shape[0] if weight.dim() == 2 else 0
    if voxels.requires_grad:
        raise _lib.LidarHipError("pillar_vfe_train: gradients with respect to the voxels are not produced (use the torch path)")
    if not pfn_train_supported(C, P, cout) or V == 0:
        raise _lib.LidarHipError(f"pillar_vfe_train: unsupported shape voxels {tuple(voxels.shape)}, cout {cout} "
                                 "(3..8 point features, P <= 64, cout <= 64, V > 0)")
    if weight.shape[1] != C + 6 + int(bool(with_distance)):
        raise _lib.LidarHipError("pillar_vfe_train: weight must be (cout, C + 6 [+1 with_distance]) — use_absolute_xyz layout")
    if any(t.dtype != torch.float32 or t.shape != (cout,) for t in (gamma, beta, running_mean, running_var)):
        raise _lib.LidarHipError(f"pillar_vfe_train: gamma, beta and the running statistics must be ({cout},) float32")
    if coords.dtype not in (torch.int32, torch.float32) or num_points.dtype not in (torch.int32, torch.float32):
        raise _lib.LidarHipError("coords / num_points must be int32 or float32")
    if num_voxels_dev is not None and num_voxels_dev.dtype != torch.int32:
        raise _lib.LidarHipError("num_voxels_dev must be an int32 device tensor")
    meta = dict(eps=float(eps), vs=_lib.host_f32(voxel_size), rng=_lib.host_f32(point_cloud_range), dist=int(bool(with_distance)),
                cf=int(coords.dtype == torch.float32), nf=int(num_points.dtype == torch.float32))
    out, batch_stats = _PillarVFETrain.apply(meta, voxels, num_points, coords, num_voxels_dev, weight, gamma, beta)
    bn_train.update_running(running_mean, running_var, num_batches_tracked, momentum, batch_stats, cout)
    if return_stats:
        return out, batch_stats[:cout], batch_stats[cout:2 * cout]
    return out


class _PillarScatterTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pillar_features, coords, num_voxels_dev, batch_size, nx, ny, channels_last):
        canvas = pillar_scatter(pillar_features, coords, batch_size, nx, ny, num_voxels_dev=num_voxels_dev, channels_last=channels_last)
        ctx.save_for_backward(coords, num_voxels_dev)
        ctx.dims = (pillar_features.shape[0], pillar_features.shape[1], batch_size, nx, ny)
        return canvas

    @staticmethod
    def backward(ctx, grad):
        coords, nvd = ctx.saved_tensors
        V, C, B, nx, ny = ctx.dims
        if grad.is_contiguous():
            nhwc = False
        elif grad.is_contiguous(memory_format=torch.channels_last):
            nhwc = True
        else:
            grad, nhwc = grad.contiguous(), False
        out = torch.empty((V, C), dtype=torch.float32, device=grad.device)
        _lib.check(_lib.lib().lidar_pillar_scatter_backward(_lib.ptr(grad), _lib.ptr(coords), int(coords.dtype == torch.float32), V,
                                                            _lib.ptr(nvd), C, B, nx, ny, int(nhwc), _lib.ptr(out), _lib.stream()),
                   "lidar_pillar_scatter_backward")
        return out, None, None, None, None, None, None


def pillar_scatter_train(pillar_features, coords, batch_size, nx, ny, num_voxels_dev=None, channels_last=False):
    """Differentiable PointPillarScatter: pillar_scatter into a FRESH canvas (autograd may still hold an earlier one), whose backward
    gathers (V, C) from the canvas gradient at the pillars' cells (NCHW or channels_last gradients; rows past the device count get
    zero).  C in {32, 64, 128}."""
    _lib.require_cuda(pillar_features, coords, num_voxels_dev)
    if pillar_features.dim() != 2 or pillar_features.shape[1] not in (32, 64, 128):
        raise _lib.LidarHipError(f"pillar_scatter_train: features must be (V, 32 | 64 | 128), got {tuple(pillar_features.shape)}")
    if coords.dtype not in (torch.int32, torch.float32) or coords.dim() != 2 or coords.shape[1] != 4:
        raise _lib.LidarHipError("pillar_scatter_train: coords must be (V, 4) [b, z, y, x] int32 or float32")
    return _PillarScatterTrain.apply(pillar_features, coords, num_voxels_dev, int(batch_size), int(nx), int(ny), bool(channels_last))
