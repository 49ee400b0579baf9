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
  * the deblocks' up-convolutions (ConvTranspose2d, kernel == stride, no bias) run on the library by default and, with
    deblock="gemm", on this package's GEMM kernels: the forward on csrc/deconv_gemm.hip (weights repacked every step) and both
    gradients on csrc/deconv_train.hip (bitwise reproducible), each direction where its kernel takes the layer and the map fits
    (deblock_conv_route / deconv_train_fits);
  * the stride-2 convolutions and everything after the backbone stay on the library.
Routing is per layer (TrainBEVBackbone.routes / wgrad_routes / deblock_conv_routes): anything the kernels do not take runs the stock
module for that layer.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, bn_train, wino, workspace
from .bev_backbone import _cl, block_layer, parse_block

_MAX_SEG = 4          # inputs of one fused call (csrc/bn_train_dev.h BT_MAX_SEG)
_MAX_C = bn_train.MAX_C


# ------------------------------------------------------------------ fused train-mode BatchNorm2d + ReLU (csrc/bn_train.hip; what it
# shares with the other fused BatchNorm routes is bn_train.py's)
def bn_supported(bn, channels=None):
    """the fused kernels take this BatchNorm2d: affine, with running statistics and a numeric momentum (momentum=None's cumulative
    average stays on torch), C % 4 == 0 and 4 <= C <= 1024.  Pure host."""
    return bn_train.supported(bn, nn.BatchNorm2d, False, channels)


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
    stats, scale_shift, batch_stats = bn_train.alloc_stats(ctot, z0.device)
    ws, wsb = bn_train.get_workspace("bn_train", z0.device, rows, ctot)
    _lib.check(_lib.lib().lidar_bn_relu_train_forward(n, ptrs, lds, offs, cs, rows, _lib.ptr(gamma), _lib.ptr(beta), float(eps),
                                                      _lib.ptr(out), y_ld, int(out_offset), _lib.ptr(stats), _lib.ptr(scale_shift),
                                                      _lib.ptr(batch_stats), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_relu_train_forward")
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
    ws, wsb = bn_train.get_workspace("bn_train", gamma.device, rows, ctot)
    _lib.check(_lib.lib().lidar_bn_relu_train_backward(n, ptrs, lds, offs, cs, rows, _lib.ptr(grad_y), g_ld, int(grad_offset),
                                                       _lib.ptr(gamma), _lib.ptr(stats), _lib.ptr(scale_shift), dptrs, _lib.ptr(d_gamma),
                                                       _lib.ptr(d_beta), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_relu_train_backward")
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
    off = 0
    for b in bns:           # BatchNorm2d's running update (momentum form), on the device
        bn_train.update_module(b, batch_stats, gamma.numel(), off)
        off += b.num_features
    return y


def bn_relu_train_rows(z, bn, residual=None):
    """bn_relu_train's form for an (N, C) feature matrix and a train-mode BatchNorm1d (sparse features): relu(bn(z)) or, with
    `residual`, relu(bn(z) + residual) on the same kernels with rows = N and row stride C (spconv.train.bn_relu_train)"""
    return bn_train.bn_relu_rows_train(z, bn, residual)


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


# ------------------------------------------------------------------ deblock up-convolution: ConvTranspose2d, kernel == stride, no bias
DEBLOCK_OPTIONS = ("library", "gemm")

# largest map (bytes, at its row stride) csrc/deconv_train.hip addresses with its 32-bit offsets (the launchers refuse 2^31 - 1 and
# more).  A list so that tests can lower it.
_DECONV_TRAIN_MAX_BYTES = [2 ** 31 - 1]


def _check_deblock(deblock, who):
    if deblock not in DEBLOCK_OPTIONS:
        raise _lib.LidarHipError(f"{who}: deblock must be one of {DEBLOCK_OPTIONS}, got {deblock!r}")
    return deblock


def deconv_train_supported(K, s, c_up):
    """the gradient kernels of csrc/deconv_train.hip take this layer: s in {1, 2, 4}, K % 8 == 0 in [16, 512], C_up % 32 == 0 in
    [32, 512].  Pure host."""
    return bool(_lib.lib().lidar_deconv_train_supported(int(K), int(s), int(c_up)))


def deconv_train_fits(B, h, w, s, x_ld, g_ld):
    """the gradient kernels can address B x h x w pixels of x_ld floats (x, dx) and the s-times upsampled gradient map of g_ld floats
    per pixel: not empty, row strides multiples of 4 floats, each map under _DECONV_TRAIN_MAX_BYTES.  Pure host arithmetic."""
    P = int(B) * int(h) * int(w)
    return (P > 0 and x_ld % 4 == 0 and g_ld % 4 == 0 and P * x_ld * 4 < _DECONV_TRAIN_MAX_BYTES[0]
            and P * s * s * g_ld * 4 < _DECONV_TRAIN_MAX_BYTES[0])


def _deconv_shapes(what, x_shape, g, weight, s):
    B, K, h, w = x_shape
    c_up = weight.shape[1]
    if tuple(weight.shape) != (K, c_up, s, s) or tuple(g.shape) != (B, c_up, s * h, s * w) or g.device != weight.device:
        raise _lib.LidarHipError(f"{what}: x {tuple(x_shape)}, weight {tuple(weight.shape)}, stride {s} and gradient {tuple(g.shape)} do not "
                                 "belong to one kernel == stride ConvTranspose2d")
    if not deconv_train_supported(K, s, c_up):
        raise _lib.LidarHipError(f"{what}: (K, s, C_up) = ({K}, {s}, {c_up}) is not supported (deconv_train_supported)")
    return B, K, h, w, c_up


def deconv_forward_gemm(x, weight, s):
    """conv_transpose2d(x, weight, stride=s) for kernel == stride == s and no bias on csrc/deconv_gemm.hip: x (B, K, h, w) channels-last,
    weight the module's (K, C_up, s, s) -> a new channels-last (B, C_up, s h, s w) map.  The weights are repacked on every call."""
    from .bev_backbone import deconv_pack
    _lib.require_nhwc(x, "deconv_forward_gemm")
    B, K, h, w = x.shape
    c_up = weight.shape[1]
    if tuple(weight.shape) != (K, c_up, s, s):
        raise _lib.LidarHipError(f"deconv_forward_gemm: weight {tuple(weight.shape)} does not match x {tuple(x.shape)} and stride {s}")
    packed = deconv_pack(weight.permute(0, 2, 3, 1).reshape(K, s * s * c_up))       # columns (ky, kx, c)
    out = torch.empty((B, c_up, s * h, s * w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _lib.check(_lib.lib().lidar_deconv_gemm_nhwc(_lib.ptr(x), B, h, w, K, _lib.ptr(packed), None, 0, int(s), c_up, _lib.ptr(out), c_up, 0,
                                                 _lib.stream()), "lidar_deconv_gemm_nhwc")
    return out


def deconv_dgrad(g, weight, s):
    """the input gradient of conv_transpose2d(x, weight, stride=s) (kernel == stride == s): g (B, C_up, s h, s w), a channels-last fp32
    map or a channel slice of one, weight (K, C_up, s, s) -> dx (B, K, h, w) channels-last.  One fixed summation order: bitwise
    reproducible; no host synchronisation (csrc/deconv_train.hip)."""
    g_ld = _lib.nhwc_ld(g, "deconv_dgrad g")
    wc = weight.contiguous()               # torch's own (K, C_up, s, s) layout (a channels-last model holds it permuted)
    _lib.require_cuda(wc)
    if g.shape[2] % s or g.shape[3] % s:
        raise _lib.LidarHipError(f"deconv_dgrad: the gradient map {tuple(g.shape)} is no multiple of the stride {s}")
    x_shape = (g.shape[0], weight.shape[0], g.shape[2] // s, g.shape[3] // s)
    B, K, h, w, c_up = _deconv_shapes("deconv_dgrad", x_shape, g, weight, s)
    if not deconv_train_fits(B, h, w, s, K, g_ld) or g.data_ptr() % 16:
        raise _lib.LidarHipError(f"deconv_dgrad: a gradient map of shape {tuple(g.shape)} is empty, misaligned or too large (deconv_train_fits)")
    dx = torch.empty((B, K, h, w), dtype=torch.float32, device=g.device, memory_format=torch.channels_last)
    _lib.check(_lib.lib().lidar_deconv_dgrad_nhwc(_lib.ptr(g), g_ld, _lib.ptr(wc), B, h, w, K, int(s), c_up, _lib.ptr(dx), K,
                                                  _lib.stream()), "lidar_deconv_dgrad_nhwc")
    return dx


def deconv_wgrad(x, g, s):
    """the weight gradient of conv_transpose2d(x, weight, stride=s) (kernel == stride == s): x (B, K, h, w) and g (B, C_up, s h, s w),
    channels-last fp32 maps or channel slices of such maps -> dW (K, C_up, s, s) fp32, contiguous.  fp32 partial sums over <= 4096
    pixels, the rest in fp64; bitwise reproducible; no host synchronisation (csrc/deconv_train.hip)."""
    x_ld, g_ld = _lib.nhwc_ld(x, "deconv_wgrad x"), _lib.nhwc_ld(g, "deconv_wgrad g")
    K, c_up = x.shape[1], g.shape[1]
    dw = torch.empty((K, c_up, s, s), dtype=torch.float32, device=x.device)
    B, K, h, w, c_up = _deconv_shapes("deconv_wgrad", x.shape, g, dw, s)
    if not deconv_train_fits(B, h, w, s, x_ld, g_ld) or x.data_ptr() % 16 or g.data_ptr() % 16:
        raise _lib.LidarHipError(f"deconv_wgrad: maps of shape {tuple(x.shape)} / {tuple(g.shape)} are empty, misaligned or too large "
                                 "(deconv_train_fits)")
    L = _lib.lib()
    wsb = L.lidar_deconv_wgrad_workspace_bytes(B, h, w, K, int(s), c_up)
    ws = workspace.get("deconv_wgrad", wsb, x.device)
    _lib.check(L.lidar_deconv_wgrad_nhwc(_lib.ptr(x), x_ld, _lib.ptr(g), g_ld, B, h, w, K, int(s), c_up, _lib.ptr(dw), _lib.ptr(ws), wsb,
                                         _lib.stream()), "lidar_deconv_wgrad_nhwc")
    return dw


class _DeconvTrain(torch.autograd.Function):
    """deblock="gemm": each direction on this package's kernel where the kernel takes the layer and the maps fit, else the library"""

    @staticmethod
    def forward(ctx, x, weight, s):
        from .bev_backbone import deconv_fits, deconv_supported
        w = weight.detach()
        ctx.save_for_backward(x, weight)
        ctx.s = s
        B, K, h, wd = x.shape
        c_up = w.shape[1]
        if deconv_supported(K, s, c_up) and deconv_fits(B, K, h, wd, s, c_up):
            return deconv_forward_gemm(x, w, s)
        return _cl(F.conv_transpose2d(x, w, None, s))

    @staticmethod
    def backward(ctx, grad_z):
        x, weight = ctx.saved_tensors
        g, w, s = _cl(grad_z), weight.detach(), ctx.s
        B, K, h, wd = x.shape
        c_up = w.shape[1]
        # decided on the host from the shapes, as the weight gradient of the 3x3 layers is (_WinoConv3x3Train.backward)
        own = (deconv_train_supported(K, s, c_up) and deconv_train_fits(B, h, wd, s, K, c_up)
               and x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0)

        def library(mask):
            return torch.ops.aten.convolution_backward(g, x, w, None, [s, s], [0, 0], [1, 1], True, [0, 0], 1, mask)

        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = deconv_dgrad(g, w, s) if own else library([True, False, False])[0]
        if ctx.needs_input_grad[1]:
            dw = deconv_wgrad(x, g, s) if own else library([False, True, False])[1]
        return dx, dw, None


def deconv_train(x, weight, stride, deblock="library"):
    """conv_transpose2d(x, weight, stride=stride) for a bias-free ConvTranspose2d with kernel == stride on a channels-last fp32 map ->
    a channels-last map.  deblock="library" (the default): torch's own call and backward.  deblock="gemm": the forward on
    csrc/deconv_gemm.hip where bev_backbone.deconv_supported / deconv_fits hold, the input and the weight gradient on
    csrc/deconv_train.hip where deconv_train_supported / deconv_train_fits hold (bitwise reproducible), the library for whatever
    they do not take; saves x and the weight only."""
    _check_deblock(deblock, "deconv_train")
    s = int(stride[0] if isinstance(stride, (tuple, list)) else stride)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (s, s) or weight.shape[0] != x.shape[1]:
        raise _lib.LidarHipError(f"deconv_train: weight {tuple(weight.shape)} is no (K, C_up, {s}, {s}) filter for x {tuple(x.shape)}")
    _lib.require_nhwc(x, "deconv_train")
    if deblock == "library":
        return _cl(F.conv_transpose2d(x, weight, None, s))
    return _DeconvTrain.apply(x, weight, s)


def deblock_conv_route(de, deblock="library"):
    """who runs (forward, input gradient, weight gradient) of one deblock's up-convolution under the option `deblock`, each "gemm"
    (csrc/deconv_gemm.hip / csrc/deconv_train.hip) or "library".  All "library" unless the option asks for "gemm" and the deblock
    opens with a bias-free ConvTranspose2d with kernel == stride, no padding, dilation or groups; then per direction by the kernels'
    supported widths.  Pure host, from the module alone; a map that does not fit the kernels' 32-bit offsets still takes the library
    at run time.  (A host-side rule that leaves a measured-slower shape on the library would live here: DESIGN 3.20.)"""
    from .bev_backbone import deconv_supported
    _check_deblock(deblock, "deblock_conv_route")
    library = ("library", "library", "library")
    mods = list(de) if isinstance(de, (nn.Sequential, list, tuple)) else [de]
    up = mods[0] if mods else None
    if deblock != "gemm" or type(up) is not nn.ConvTranspose2d:
        return library
    s = up.stride[0]
    if (up.bias is not None or tuple(up.kernel_size) != (s, s) or tuple(up.stride) != (s, s) or tuple(up.padding) != (0, 0)
            or tuple(up.output_padding) != (0, 0) or tuple(up.dilation) != (1, 1) or up.groups != 1):
        return library
    K, c_up = up.in_channels, up.out_channels
    grad = "gemm" if deconv_train_supported(K, s, c_up) else "library"
    return ("gemm" if deconv_supported(K, s, c_up) else "library", grad, grad)


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
    gradients of the "wino"-routed layers ("library", the default, or "wino": see wgrad_routes).  deblock: who runs the deblocks'
    up-convolutions ("library", the default, or "gemm": see deblock_conv_routes)."""

    def __init__(self, blocks, deblocks, wgrad="library", deblock="library"):
        self.wgrad = _check_wgrad(wgrad, "TrainBEVBackbone")
        self.deblock = _check_deblock(deblock, "TrainBEVBackbone")
        self.blocks, self.deblocks = list(blocks), list(deblocks)
        self.plan = []
        for blk in self.blocks:
            layers = parse_block(blk)
            self.plan.append(("stock", blk) if layers is None else ("layers", [(_route(l), l) for l in layers]))
        n = len(self.blocks)
        self.de_routes = [deblock_route(de) for de in self.deblocks[:n]]
        # a "stock" deblock runs as the module it is: its up-convolution stays on the library whatever the option says
        self.de_conv_routes = [deblock_conv_route(de, self.deblock) if r == "fused" else ("library",) * 3
                               for de, r in zip(self.deblocks[:n], self.de_routes)]
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

    def deblock_conv_routes(self):
        """-> [(forward, input gradient, weight gradient) of each deblock's up-convolution], each "gemm" (csrc/deconv_gemm.hip /
        csrc/deconv_train.hip) or "library" (deblock_conv_route; all "library" for a deblock routes() calls "stock")"""
        return list(self.de_conv_routes)

    def _up(self, i, f):
        """deblock i's up-convolution of the block output f"""
        up = list(self.deblocks[i])[0]
        if "gemm" in self.de_conv_routes[i]:
            return deconv_train(f, up.weight, up.stride[0], "gemm")
        return _cl(up(f))

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
            zs = [self._up(i, f) for i, f in enumerate(feats)]
            out = bn_relu_train(zs, [list(de)[1] for de in self.deblocks[:n]])
        else:
            ups = []
            for i, (de, f, route) in enumerate(zip(self.deblocks, feats, self.de_routes)):
                ups.append(bn_relu_train(self._up(i, f), list(de)[1]) if route == "fused" else _cl(de(f)))
            out = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
        if self.extra is not None:
            out = _cl(self.extra(out))
        return (out, feats) if return_blocks else out
