"""SparseConvTensor (spconv/__init__.py upstream; ctor call site pcdet/models/backbones_3d/spconv_backbone.py:132-137)."""
import torch

from .. import _lib, workspace


def _nhwc_slice_ld(g):
    """row stride (floats) of a (B, C, H, W) fp32 CUDA gradient that is a channels-last map or a channel slice of one, else None"""
    if not (g.is_cuda and g.dtype == torch.float32 and g.dim() == 4):
        return None
    B, Cc, H, W = g.shape
    ld = g.stride(3)
    if g.stride(1) != 1 or ld < Cc or g.stride(2) != W * ld or g.stride(0) != H * W * ld:
        return None
    return ld


def dense_bev_backward(grad, indices, channels, D, offset=0):
    """the gradient of SparseConvTensor.dense_bev() with respect to the features (csrc/sparse_train.hip): grad is the gradient of the
    (B, channels * D, H, W) BEV map, channels-last (or a channel slice of a wider channels-last map), or a wider channels-last map
    whose channels [offset, offset + channels * D) are that gradient; indices (n, 4) int32 [b, z, y, x] as the forward took them
    -> (n, channels) with d_features[row][c] = grad[b][c * D + z][y][x]; exactly 0 for a row outside the volume.  A pure gather: no
    atomics, no workspace, bitwise equal to the stock index_put backward.  channels % 4 == 0, 1 <= D <= 4."""
    ld = _nhwc_slice_ld(grad)
    if ld is None:
        grad = grad.contiguous(memory_format=torch.channels_last)
        ld = _nhwc_slice_ld(grad)
        if ld is None:
            raise _lib.LidarHipError(f"dense_bev_backward: expected a 4-d float32 CUDA gradient, got {grad.dtype} {tuple(grad.shape)}")
    B, ctot, H, W = grad.shape
    n = int(indices.shape[0])
    if channels % 4 or not 1 <= D <= 4 or offset < 0 or offset + channels * D > ctot:
        raise _lib.LidarHipError(f"dense_bev_backward: channels {channels}, D {D}, offset {offset} do not fit a {ctot}-channel gradient")
    idx = indices.int().contiguous()
    out = torch.empty((n, channels), dtype=torch.float32, device=grad.device)
    if n:
        _lib.check(_lib.lib().lidar_sparse_to_bev_nhwc_backward(_lib.ptr(grad), int(ld), int(offset), _lib.ptr(idx), n, int(channels), B,
                                                                int(D), H, W, _lib.ptr(out), _lib.stream()),
                   "lidar_sparse_to_bev_nhwc_backward")
    return out


class _DenseBEV(torch.autograd.Function):
    """HeightCompression on the one-pass kernels: lidar_sparse_to_bev_nhwc forward, lidar_sparse_to_bev_nhwc_backward backward; both
    are copies, so values and gradients equal the stock index_put path bit for bit"""

    @staticmethod
    def forward(ctx, feats, idx, B, D, H, W):
        ctx.save_for_backward(idx)
        ctx.dims = (feats.shape[1], D)
        return _bev_forward(feats, idx, B, D, H, W)

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        C, D = ctx.dims
        return dense_bev_backward(grad, idx, C, D), None, None, None, None, None


def _bev_forward(feats, idx, B, D, H, W):
    N, C = feats.shape
    L = _lib.lib()
    out = torch.empty((B, C * D, H, W), dtype=torch.float32, device=feats.device, memory_format=torch.channels_last)
    wsb = L.lidar_sparse_to_dense_workspace_bytes(B, D, H, W)
    ws = workspace.get("dense", wsb, feats.device)
    _lib.check(L.lidar_sparse_to_bev_nhwc(_lib.ptr(feats), _lib.ptr(idx), N, C, B, D, H, W, _lib.ptr(out), _lib.ptr(ws), wsb,
                                          _lib.stream()), "lidar_sparse_to_bev_nhwc")
    return out


class SparseConvTensor(object):
    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        """features (N, C) f32; indices (N, 4) int32 [b, z, y, x]; spatial_shape [D, H, W]."""
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {}
        self.grid = grid

    @property
    def spatial_size(self):
        n = 1
        for s in self.spatial_shape:
            n *= s
        return n

    def find_indice_pair(self, key):
        if key is None:
            return None
        return self.indice_dict.get(key, None)

    def dense(self, channels_first=True):
        """(N, C) rows -> dense (B, C, D, H, W) [channels_first] or (B, D, H, W, C); zeros elsewhere."""
        feats = self.features.contiguous()
        N, C = feats.shape
        B, (D, H, W) = self.batch_size, self.spatial_shape
        if C in (32, 64, 128) and feats.dtype == torch.float32 and feats.is_cuda and not feats.requires_grad:
            L = _lib.lib()
            out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=feats.device)
            wsb = L.lidar_sparse_to_dense_workspace_bytes(B, D, H, W)
            ws = workspace.get("dense", wsb, feats.device)
            idx = self.indices.int().contiguous()
            _lib.check(L.lidar_sparse_to_dense(_lib.ptr(feats), _lib.ptr(idx), N, C, B, D, H, W, _lib.ptr(out), _lib.ptr(ws), wsb,
                                               _lib.stream()), "lidar_sparse_to_dense")
            return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()
        # differentiable / odd-width path: index_put on a zero volume (stock torch)
        out = feats.new_zeros((B, D, H, W, C))
        idx = self.indices.long()
        out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = feats
        return out.permute(0, 4, 1, 2, 3).contiguous() if channels_first else out

    def dense_bev(self):
        """HeightCompression in one pass: (B, C*D, H, W) with channels-last strides, equal to
        dense().view(B, C*D, H, W).contiguous(memory_format=torch.channels_last) (height_compression.py:21-24).  Differentiable with
        respect to the features on the same kernels (forward and gradient are copies: bitwise equal to that expression's)."""
        feats = self.features.contiguous()
        N, C = feats.shape
        B, (D, H, W) = self.batch_size, self.spatial_shape
        grad = feats.requires_grad and torch.is_grad_enabled()
        # an empty tensor that needs a gradient stays on the stock path, as every tensor that needed one did
        if not (feats.is_cuda and feats.dtype == torch.float32 and C % 4 == 0 and D <= 4) or (grad and N == 0):
            d = self.dense()
            return d.view(B, C * D, H, W).contiguous(memory_format=torch.channels_last)
        idx = self.indices.int().contiguous()
        if grad:
            return _DenseBEV.apply(feats, idx, B, D, H, W)
        return _bev_forward(feats.detach(), idx, B, D, H, W)

    @property
    def sparity(self):
        return self.indices.shape[0] / self.spatial_size / self.batch_size
