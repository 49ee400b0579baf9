"""Train-mode dense BEV backbone on this package's kernels (the training counterpart of bev_backbone.FoldedBEVBackbone).

reference: pcdet/models/backbones_2d/base_bev_backbone.py:31-69 (ZeroPad2d / Conv2d / BatchNorm2d / ReLU blocks, ConvTranspose2d
deblocks), :81-112 (forward, torch.cat of the deblock outputs).

In training, BatchNorm2d normalises with the statistics of the batch itself, so it cannot be folded into the convolution as the
inference path does.  What runs here instead:
  * every supported BatchNorm2d + ReLU pair is ONE fused train-mode kernel sequence forward and one backward (csrc/bn_train.hip):
    fp64 batch statistics, y = relu(BN(z)) in one pass, the backward recomputes the ReLU mask from z (no mask or y is saved);
    the deblocks' three pairs are one call whose output IS the concatenated map (no torch.cat, no split of its gradient);
  * stride-1 3x3 convolutions run forward on the Winograd kernels (wino.conv3x3_auto's routing: F(4x4, 3x3) in csrc/wino43_conv.hip,
    F(2x2, 3x3) in csrc/wino_conv.hip for maps too large for F(4x4)), and so does their input gradient: a stride-1, pad-1 3x3
    convolution of the output gradient with the filters flipped by 180 degrees and Cin / Cout swapped (repacked every step);
  * their weight gradient runs on the library by default (torch.ops.aten.convolution_backward, MIOpen: split-K with float atomics,
    not bitwise reproducible) and, with wgrad="wino", on the Winograd F(3x3, 4x4) weight-gradient kernel (csrc/wino43_wgrad.hip,
    wino.conv3x3_wgrad_f43: bitwise reproducible) for every layer it supports and whose map fits (wgrad_route / wino.wgrad43_fits);
  * the stride-2 convolutions, the deblock convolutions and everything after the backbone stay on the library.
Routing is per layer (TrainBEVBackbone.routes / wgrad_routes): anything the kernels do not take runs the stock module for that layer.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, wino, workspace
from .bev_backbone import _cl, block_layer, parse_block

_MAX_SEG = 4          # inputs of one fused call (csrc/bn_train.hip BT_MAX_SEG)
_MAX_C = 1024         # channels of one input (BT_MAX_C)


# ------------------------------------------------------------------ fused train-mode BatchNorm2d + ReLU (csrc/bn_train.hip)
def bn_supported(bn, channels=None):
    """the fused kernels take this BatchNorm2d: affine, with running statistics and a numeric momentum (momentum=None's cumulative
    average stays on torch), C % 4 == 0 and 4 <= C <= 1024.  Pure host."""
    if not isinstance(bn, nn.BatchNorm2d):
        return False
    c = bn.num_features if channels is None else int(channels)
    return (bn.affine and bn.track_running_stats and bn.running_mean is not None and bn.num_batches_tracked is not None
            and isinstance(bn.momentum, (int, float)) and not isinstance(bn.momentum, bool)
            and c == bn.num_features and c % 4 == 0 and 4 <= c <= _MAX_C)


def _segments(zs):
    zs = list(zs)
    if not 1 <= len(zs) <= _MAX_SEG:
        raise _lib.LidarHipError(f"bn_relu: 1..{_MAX_SEG} inputs per call, got {len(zs)}")
    B, _, H, W = zs[0].shape
    lds = []
    for z in zs:
        lds.append(_lib.nhwc_ld(z, "bn_relu input"))
        if z.shape[0] != B or tuple(z.shape[2:]) != (H, W):
            raise _lib.LidarHipError("bn_relu: every input must have the same batch and spatial shape")
        if z.shape[1] % 4 or not 4 <= z.shape[1] <= _MAX_C:
            raise _lib.LidarHipError(f"bn_relu: channels must be a multiple of 4 in [4, {_MAX_C}], got {z.shape[1]}")
    n = len(zs)
    ptrs = (C.c_void_p * n)(*[z.data_ptr() for z in zs])
    return (n, ptrs, _lib.host_i32(lds), _lib.host_i32([0] * n), _lib.host_i32([z.shape[1] for z in zs]), B * H * W,
            sum(int(z.shape[1]) for z in zs))


def bn_relu_forward(zs, gamma, beta, eps, out=None, out_offset=0):
    """y = relu(batch_norm(cat(zs), training=True)) for channels-last maps zs (each a map or a channel slice of one; C % 4 == 0):
    -> (y, stats, scale_shift, batch_stats).  y is a new channels-last (B, sum C, H, W) map, or `out` (channels-last, written at
    channels [out_offset, out_offset + sum C)).  stats / scale_shift feed bn_relu_backward; batch_stats = (mean | biased variance |
    unbiased variance), 3 * sum C floats.  No host synchronisation."""
    _lib.require_cuda(gamma, beta)
    n, ptrs, lds, offs, cs, rows, ctot = _segments(zs)
    if gamma.numel() != ctot or beta.numel() != ctot:
        raise _lib.LidarHipError(f"bn_relu_forward: gamma / beta must hold {ctot} values")
    z0 = zs[0]
    B, _, H, W = z0.shape
    out, out_offset = _lib.nhwc_out("bn_relu_forward", B, (H, W), ctot, z0.device, out, out_offset, sliced=True)
    y_ld = out.stride(3)
    dev = z0.device
    stats = torch.empty(2 * ctot, dtype=torch.float64, device=dev)
    scale_shift = torch.empty(2 * ctot, dtype=torch.float32, device=dev)
    batch_stats = torch.empty(3 * ctot, dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.lidar_bn_relu_train_workspace_bytes(rows, ctot)
    ws = workspace.get("bn_train", wsb, dev)
    _lib.check(L.lidar_bn_relu_train_forward(n, ptrs, lds, offs, cs, rows, _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(out),
                                             y_ld, int(out_offset), _lib.ptr(stats), _lib.ptr(scale_shift), _lib.ptr(batch_stats),
                                             _lib.ptr(ws), wsb, _lib.stream()), "lidar_bn_relu_train_forward")
    return out, stats, scale_shift, batch_stats


def bn_relu_backward(zs, grad_y, gamma, stats, scale_shift, grad_offset=0):
    """the backward of bn_relu_forward: grad_y is the gradient of its output (channels-last; the inputs' channels start at
    grad_offset) -> ([dz per input, laid out like its z: a channel slice of a z-wide buffer when z is a slice], d_gamma, d_beta)"""
    _lib.require_cuda(gamma, scale_shift)
    n, ptrs, lds, offs, cs, rows, ctot = _segments(zs)
    g_ld = _lib.nhwc_ld(grad_y, "bn_relu_backward grad")
    if grad_y.shape[0] != zs[0].shape[0] or grad_y.shape[2:] != zs[0].shape[2:] or not 0 <= grad_offset <= grad_y.shape[1] - ctot:
        raise _lib.LidarHipError("bn_relu_backward: the gradient must be (B, >= grad_offset + sum C, H, W)")
    dzs = []
    for z, ld in zip(zs, lds):      # dz is written at its z's row stride
        B, c, H, W = z.shape
        buf = torch.empty((B, ld, H, W), dtype=torch.float32, device=z.device, memory_format=torch.channels_last)
        dzs.append(buf if ld == c else buf[:, :c])
    d_gamma = torch.empty(ctot, dtype=torch.float32, device=gamma.device)
    d_beta = torch.empty(ctot, dtype=torch.float32, device=gamma.device)
    dptrs = (C.c_void_p * n)(*[d.data_ptr() for d in dzs])
    L = _lib.lib()
    wsb = L.lidar_bn_relu_train_workspace_bytes(rows, ctot)
    ws = workspace.get("bn_train", wsb, gamma.device)
    _lib.check(L.lidar_bn_relu_train_backward(n, ptrs, lds, offs, cs, rows, _lib.ptr(grad_y), g_ld, int(grad_offset), _lib.ptr(gamma),
                                              _lib.ptr(stats), _lib.ptr(scale_shift), dptrs, _lib.ptr(d_gamma), _lib.ptr(d_beta),
                                              _lib.ptr(ws), wsb, _lib.stream()), "lidar_bn_relu_train_backward")
    return dzs, d_gamma, d_beta


class _BNReLUTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eps, gamma, beta, *zs):
        y, stats, scale_shift, batch_stats = bn_relu_forward(zs, gamma, beta, eps)
        ctx.save_for_backward(gamma, stats, scale_shift, *zs)          # z only: y and the ReLU mask are recomputed
        ctx.mark_non_differentiable(batch_stats)
        return y, batch_stats

    @staticmethod
    def backward(ctx, grad_y, _grad_stats):
        gamma, stats, scale_shift, *zs = ctx.saved_tensors
        dzs, d_gamma, d_beta = bn_relu_backward(zs, _cl(grad_y), gamma, stats, scale_shift)
        need = ctx.needs_input_grad
        return (None, d_gamma if need[1] else None, d_beta if need[2] else None,
                *[d if need[3 + i] else None for i, d in enumerate(dzs)])


def bn_relu_train(z, bn):
    """relu(bn(z)) for train-mode BatchNorm2d module(s) `bn` on channels-last fp32 map(s) `z`, differentiable with respect to z and
    the modules' weight / bias; the modules' running_mean / running_var / num_batches_tracked are updated in place as BatchNorm2d
    does (torch ops on the device-computed batch statistics: their version counters move, so a FoldedBEVBackbone built from the
    modules refolds).  A list of maps and the same number of modules (one eps): one fused call whose output is the concatenated
    map, channels in list order.  No host synchronisation."""
    zs = list(z) if isinstance(z, (list, tuple)) else [z]
    bns = list(bn) if isinstance(bn, (list, tuple)) else [bn]
    if len(zs) != len(bns):
        raise _lib.LidarHipError("bn_relu_train: one BatchNorm2d per input")
    for zi, b in zip(zs, bns):
        if not bn_supported(b, zi.shape[1]):
            raise _lib.LidarHipError(f"bn_relu_train: unsupported BatchNorm2d / width {zi.shape[1]} (bn_supported)")
    if len({float(b.eps) for b in bns}) != 1:
        raise _lib.LidarHipError("bn_relu_train: the modules of one call must share eps")
    if len(bns) == 1:
        gamma, beta = bns[0].weight, bns[0].bias
    else:
        gamma, beta = torch.cat([b.weight for b in bns]), torch.cat([b.bias for b in bns])
    y, batch_stats = _BNReLUTrain.apply(float(bns[0].eps), gamma, beta, *zs)
    ctot = gamma.numel()
    with torch.no_grad():   # BatchNorm2d's running update (momentum form), on the device
        off = 0
        for b in bns:
            c, m = b.num_features, float(b.momentum)
            b.running_mean.mul_(1.0 - m).add_(batch_stats[off:off + c], alpha=m)
            b.running_var.mul_(1.0 - m).add_(batch_stats[2 * ctot + off:2 * ctot + off + c], alpha=m)
            b.num_batches_tracked.add_(1)
            off += c
    return y


# ------------------------------------------------------------------ stride-1 3x3 convolution on the Winograd kernels
def wino_train_supported(cin, cout):
    """both directions run on the Winograd kernels: the forward (Cin -> Cout) and the input gradient (Cout -> Cin).  Pure host."""
    return wino.supported(cin, cout) and wino.supported(cout, cin)


def _wino(x, w):
    """conv3x3(x, w, padding=1) with no bias or ReLU on the kernel wino.kernel_for names for this layer and map (the filters are
    repacked every step: only those the chosen kernel reads)"""
    cout, cin = w.shape[:2]
    if wino.kernel_for(cin, cout, x.shape) == "f43":
        return wino.conv3x3_f43(x, wino.pack_weights43(w), cout, None, relu=False)
    return wino.conv3x3(x, wino.pack_weights(w), cout, None, relu=False)


WGRAD_OPTIONS = ("library", "wino")


def _check_wgrad(wgrad, who):
    if wgrad not in WGRAD_OPTIONS:
        raise _lib.LidarHipError(f"{who}: wgrad must be one of {WGRAD_OPTIONS}, got {wgrad!r}")
    return wgrad


def wgrad_route(cin, cout, wgrad="library"):
    """who computes the weight gradient of a Winograd-routed (Cin -> Cout) layer under the option `wgrad`: "wino" (the F(3x3, 4x4)
    kernel) when the option asks for it and the kernel supports the widths, else "library".  Pure host.  (A host-side rule that
    leaves a measured-slower shape on the library would live here; none is needed: DESIGN 3.17.)"""
    _check_wgrad(wgrad, "wgrad_route")
    return "wino" if wgrad == "wino" and wino.wgrad43_supported(cin, cout) else "library"


class _WinoConv3x3Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, wgrad="library"):
        w = weight.detach()
        ctx.save_for_backward(x, weight)
        ctx.wgrad = wgrad
        return _wino(x, w)

    @staticmethod
    def backward(ctx, grad_z):
        x, weight = ctx.saved_tensors
        g = _cl(grad_z)
        dx = dw = None
        if ctx.needs_input_grad[0]:    # dx = conv3x3(g, flip(w) with Cin / Cout swapped, padding=1): the same kernels
            dx = _wino(g, weight.detach().flip(2, 3).transpose(0, 1))
        if ctx.needs_input_grad[1]:
            cout, cin = weight.shape[:2]
            # decided on the host from the shapes: the kernel where the option asks for it, the widths are supported and the maps
            # fit its 32-bit offsets; the library (MIOpen) otherwise
            if wgrad_route(cin, cout, ctx.wgrad) == "wino" and wino.wgrad43_fits(x.shape, cout):
                dw = wino.conv3x3_wgrad_f43(x, g)
            else:
                dw = torch.ops.aten.convolution_backward(g, x, weight.detach(), None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                         [False, True, False])[1]
        return dx, dw, None


def conv3x3_train(x, weight, wgrad="library"):
    """conv2d(x, weight, stride=1, padding=1) (no bias) on a channels-last fp32 map, forward and input gradient on the Winograd
    kernels; weight gradient on the library (wgrad="library", the default) or on the Winograd weight-gradient kernel where it takes
    the layer (wgrad="wino"); saves x only"""
    _check_wgrad(wgrad, "conv3x3_train")
    if not wino_train_supported(weight.shape[1], weight.shape[0]):
        raise _lib.LidarHipError(f"conv3x3_train: (Cout, Cin) = {tuple(weight.shape[:2])} is not taken by the Winograd kernels in both directions")
    _lib.require_nhwc(x, "conv3x3_train")
    return _WinoConv3x3Train.apply(x, weight, wgrad)


# ------------------------------------------------------------------ the backbone
def _route(l):
    """conv_route of a bev_backbone.BlockLayer"""
    conv = l.conv
    if (type(conv) is not nn.Conv2d or not bn_supported(l.bn, conv.out_channels) or l.pad is None or l.zero_pad is not None
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1):
        return "stock"
    if l.plain3x3 and conv.bias is None and wino_train_supported(conv.in_channels, conv.out_channels):
        return "wino"
    return "conv"


def conv_route(conv, bn, zero_pad=(0, 0, 0, 0)):
    """how TrainBEVBackbone runs one Conv2d -> BatchNorm2d -> ReLU layer (preceded by ZeroPad2d(zero_pad), or not): "wino" (Winograd
    forward and input gradient + fused BN / ReLU), "conv" (stock F.conv2d on the folded padding + fused BN / ReLU) or "stock" (the
    modules themselves).  Pure host."""
    if not isinstance(conv, nn.Conv2d):
        return "stock"
    return _route(block_layer(nn.ZeroPad2d(tuple(int(v) for v in zero_pad)), conv, bn))


def deblock_route(de):
    """"fused" (stock up-convolution + the fused BN / ReLU into the concatenated map) or "stock" for one deblock.  Pure host."""
    mods = list(de)
    if len(mods) != 3 or not isinstance(mods[2], nn.ReLU) or not isinstance(mods[0], (nn.ConvTranspose2d, nn.Conv2d)):
        return "stock"
    return "fused" if bn_supported(mods[1], mods[0].out_channels) else "stock"


class TrainBEVBackbone:
    """BaseBEVBackbone's train-mode forward on the reference-shaped modules themselves (`blocks`, `deblocks` as
    pointpillar.make_bev_backbone / the reference build them): their parameters receive the gradients and their BatchNorm running
    statistics are updated.  Call with the channels-last fp32 BEV map -> the concatenated deblock map (channels-last); autograd
    does the backward.  Building it is pure host (routes are decided from the modules' settings).  wgrad: who computes the weight
    gradients of the "wino"-routed layers ("library", the default, or "wino": see wgrad_routes)."""

    def __init__(self, blocks, deblocks, wgrad="library"):
        self.wgrad = _check_wgrad(wgrad, "TrainBEVBackbone")
        self.blocks, self.deblocks = list(blocks), list(deblocks)
        self.plan = []
        for blk in self.blocks:
            layers = parse_block(blk)
            self.plan.append(("stock", blk) if layers is None else ("layers", [(_route(l), l) for l in layers]))
        n = len(self.blocks)
        self.de_routes = [deblock_route(de) for de in self.deblocks[:n]]
        self.extra = self.deblocks[n] if len(self.deblocks) > n else None       # a final deblock on the concatenated map (stock)
        bns = [list(de)[1] for de in self.deblocks[:n]]
        self.de_merged = (len(bns) > 0 and all(r == "fused" for r in self.de_routes) and len(bns) <= _MAX_SEG
                          and len({float(b.eps) for b in bns}) == 1)

    def routes(self):
        """-> [[route of each layer] per block], [route of each deblock]  (a block of unknown structure: ["stock"])"""
        return ([[route for route, _ in steps] if kind == "layers" else ["stock"] for kind, steps in self.plan], list(self.de_routes))

    def wgrad_routes(self):
        """-> [[who computes each layer's weight gradient] per block]: "wino" (csrc/wino43_wgrad.hip), "library" (MIOpen), or None for
        a layer that is not on the Winograd route at all (routes() != "wino": autograd's own backward).  From the widths alone; a
        "wino" layer whose map does not fit the kernel's 32-bit offsets (wino.wgrad43_fits) still takes the library at run time."""
        return [[(wgrad_route(l.conv.in_channels, l.conv.out_channels, self.wgrad) if route == "wino" else None) for route, l in steps]
                if kind == "layers" else [None] for kind, steps in self.plan]

    def _layer(self, step, x):
        route, l = step
        if route == "stock":
            return _cl(l.act(l.bn(l.conv(x if l.zpad is None else l.zpad(x)))))
        if route == "wino":
            z = conv3x3_train(x, l.conv.weight, self.wgrad)
        else:
            z = _cl(F.conv2d(x, l.conv.weight, l.conv.bias, l.conv.stride, l.pad))
        return bn_relu_train(z, l.bn)

    def __call__(self, x, return_blocks=False):
        """x (B, C, H, W) channels-last fp32 CUDA -> the concatenated map; return_blocks: (map, [each block's output])"""
        _lib.require_nhwc(x, "TrainBEVBackbone")
        feats = []
        for kind, steps in self.plan:
            if kind == "stock":
                x = _cl(steps(x))
            else:
                for st in steps:
                    x = self._layer(st, x)
            feats.append(x)
        n = len(self.blocks)
        if not self.deblocks[:n]:
            out = torch.cat(feats, dim=1) if len(feats) > 1 else feats[0]
        elif self.de_merged:     # every deblock's BN + ReLU in one call, written straight into the concatenated map
            zs = [_cl(list(de)[0](f)) for de, f in zip(self.deblocks, feats)]
            out = bn_relu_train(zs, [list(de)[1] for de in self.deblocks[:n]])
        else:
            ups = []
            for de, f, route in zip(self.deblocks, feats, self.de_routes):
                up, bn = list(de)[0], list(de)[1]
                ups.append(bn_relu_train(_cl(up(f)), bn) if route == "fused" else _cl(de(f)))
            out = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
        if self.extra is not None:
            out = _cl(self.extra(out))
        return (out, feats) if return_blocks else out
