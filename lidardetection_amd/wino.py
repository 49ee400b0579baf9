"""Host side of csrc/wino_conv.hip and csrc/wino43_conv.hip: the stride-1 3x3 convolutions of the dense BEV backbone
(pcdet/models/backbones_2d/base_bev_backbone.py:34-45) as Winograd F(2x2, 3x3) / F(4x4, 3x3) on the fp32 matrix cores, shift + ReLU in
the kernels' epilogue; and of csrc/wino43_wgrad.hip: the same layers' weight gradient as Winograd F(3x3, 4x4) (conv3x3_wgrad_f43)."""
import os

import torch

from . import _lib

# which Winograd kernel the model code gets for a layer both support: 1 (default) = F(4x4, 3x3) (csrc/wino43_conv.hip: fewer MFMA
# cycles, |error| ~ 1e-5 of the output scale), 0 = F(2x2, 3x3) everywhere (csrc/wino_conv.hip: ~ 2e-6).  A/B switch.
_F43 = [os.environ.get("LIDAR_WINO_F43", "1") != "0"]
# the F(4x4, 3x3) kernel's workgroup shape for layers with Cout % 128 == 0: 1 (default) = one tile group x four blocks of 32 output
# channels (input transform and region DMA once per 128 output channels; own packed filter layout), 0 = two tile groups x two blocks
# everywhere.  Bit-identical results.  A/B switch, read when the filters are packed (pack_auto).
_F43_SHARE = [os.environ.get("LIDAR_WINO43_SHARE", "1") != "0"]


def supported(cin, cout):
    return bool(_lib.lib().lidar_wino_supported(int(cin), int(cout)))


def pack_weights(w):
    """w (Cout, Cin, 3, 3) fp32 (BatchNorm scale folded in) -> the packed transformed filters the kernel reads (16 Cin Cout floats)"""
    _lib.require_cuda(w.contiguous())
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.dtype != torch.float32 or not supported(w.shape[1], w.shape[0]):
        raise _lib.LidarHipError(f"wino.pack_weights: expected a float32 (Cout % 32 == 0, Cin % 8 == 0, Cin >= 16, 3, 3) weight, got {tuple(w.shape)}")
    wc = w.detach().contiguous()                      # plain (Cout, Cin, 3, 3) order whatever the memory format of `w`
    if wc.stride() != (wc.shape[1] * 9, 9, 3, 1):
        wc = wc.clone(memory_format=torch.contiguous_format)
    L = _lib.lib()
    packed = torch.empty(L.lidar_wino_packed_floats(w.shape[1], w.shape[0]), dtype=torch.float32, device=w.device)
    _lib.check(L.lidar_wino_pack_weights(_lib.ptr(wc), w.shape[1], w.shape[0], _lib.ptr(packed), _lib.stream()), "lidar_wino_pack_weights")
    return packed


def conv3x3(x, packed, cout, bias=None, relu=True, out=None, out_offset=0):
    """x (B, Cin, H, W) channels-last fp32 -> act(conv3x3(x, w, padding=1) + bias) as a channels-last (B, cout, H, W) tensor, or
    into channels [out_offset, out_offset + cout) of the channels-last `out` (B, C_out, H, W)."""
    _lib.require_cuda(packed, bias)
    _lib.require_nhwc(x, "wino.conv3x3")
    B, cin, H, W = x.shape
    L = _lib.lib()
    if packed.numel() != L.lidar_wino_packed_floats(cin, cout) or packed.numel() == 0:
        raise _lib.LidarHipError("wino.conv3x3: packed filters do not match (Cin, Cout)")
    if bias is not None and bias.numel() != cout:
        raise _lib.LidarHipError("wino.conv3x3: bias must hold Cout values")
    out, out_offset = _lib.nhwc_out("wino.conv3x3", B, (H, W), cout, x.device, out, out_offset)
    _lib.check(L.lidar_wino_conv3x3_nhwc(_lib.ptr(x), B, H, W, cin, _lib.ptr(packed), _lib.ptr(bias), int(bool(relu)), int(cout),
                                         _lib.ptr(out), out.shape[1], int(out_offset), _lib.stream()), "lidar_wino_conv3x3_nhwc")
    return out


def supported43(cin, cout):
    """the F(4x4, 3x3) kernel (csrc/wino43_conv.hip) takes this layer: Cin % 16 == 0, Cin >= 32, Cout % 64 == 0"""
    return bool(_lib.lib().lidar_wino43_supported(int(cin), int(cout)))


def pack_weights43(w):
    """w (Cout, Cin, 3, 3) fp32 -> the packed F(4x4, 3x3) filters (36 Cin Cout floats; the filter transform runs in fp64)"""
    _lib.require_cuda(w.contiguous())
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.dtype != torch.float32 or not supported43(w.shape[1], w.shape[0]):
        raise _lib.LidarHipError(f"wino.pack_weights43: expected a float32 (Cout % 64 == 0, Cin % 16 == 0, 3, 3) weight, got {tuple(w.shape)}")
    wc = w.detach().contiguous()
    if wc.stride() != (wc.shape[1] * 9, 9, 3, 1):
        wc = wc.clone(memory_format=torch.contiguous_format)
    L = _lib.lib()
    packed = torch.empty(L.lidar_wino43_packed_floats(w.shape[1], w.shape[0]), dtype=torch.float32, device=w.device)
    _lib.check(L.lidar_wino43_pack_weights(_lib.ptr(wc), w.shape[1], w.shape[0], _lib.ptr(packed), _lib.stream()), "lidar_wino43_pack_weights")
    return packed


def supported43_share(cin, cout):
    """the shared-transform shape of the F(4x4, 3x3) kernel takes this layer: Cin % 16 == 0, Cin >= 32, Cout % 128 == 0"""
    return bool(_lib.lib().lidar_wino43s_supported(int(cin), int(cout)))


def pack_weights43_share(w):
    """pack_weights43 in the filter order of the shared-transform shape (conv3x3_f43(..., share=True)); the tensor carries the
    mark `w43_share` by which conv3x3_auto tells the two layouts apart"""
    _lib.require_cuda(w.contiguous())
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.dtype != torch.float32 or not supported43_share(w.shape[1], w.shape[0]):
        raise _lib.LidarHipError(f"wino.pack_weights43_share: expected a float32 (Cout % 128 == 0, Cin % 16 == 0, 3, 3) weight, got {tuple(w.shape)}")
    wc = w.detach().contiguous()
    if wc.stride() != (wc.shape[1] * 9, 9, 3, 1):
        wc = wc.clone(memory_format=torch.contiguous_format)
    L = _lib.lib()
    packed = torch.empty(L.lidar_wino43s_packed_floats(w.shape[1], w.shape[0]), dtype=torch.float32, device=w.device)
    _lib.check(L.lidar_wino43s_pack_weights(_lib.ptr(wc), w.shape[1], w.shape[0], _lib.ptr(packed), _lib.stream()), "lidar_wino43s_pack_weights")
    packed.w43_share = True
    return packed


def conv3x3_f43(x, packed, cout, bias=None, relu=True, out=None, out_offset=0, cin=None, share=False):
    """conv3x3 through the F(4x4, 3x3) kernel.  cin: the layer reads channels [0, cin) of x (default: all of them).  share: the
    shared-transform workgroup shape, `packed` from pack_weights43_share (bit-identical results)."""
    _lib.require_cuda(packed, bias)
    _lib.require_nhwc(x, "wino.conv3x3_f43")
    B, in_c, H, W = x.shape
    cin = in_c if cin is None else int(cin)
    L = _lib.lib()
    if bool(share) != bool(getattr(packed, "w43_share", False)):
        raise _lib.LidarHipError("wino.conv3x3_f43: filters packed for the other workgroup shape (pack_weights43 / pack_weights43_share)")
    size, run, name = ((L.lidar_wino43s_packed_floats, L.lidar_wino43s_conv3x3_nhwc, "lidar_wino43s_conv3x3_nhwc") if share else
                       (L.lidar_wino43_packed_floats, L.lidar_wino43_conv3x3_nhwc, "lidar_wino43_conv3x3_nhwc"))
    if cin > in_c or packed.numel() != size(cin, cout) or packed.numel() == 0:
        raise _lib.LidarHipError("wino.conv3x3_f43: packed filters do not match (Cin, Cout)")
    if bias is not None and bias.numel() != cout:
        raise _lib.LidarHipError("wino.conv3x3_f43: bias must hold Cout values")
    out, out_offset = _lib.nhwc_out("wino.conv3x3_f43", B, (H, W), cout, x.device, out, out_offset)
    _lib.check(run(_lib.ptr(x), B, H, W, cin, in_c, _lib.ptr(packed), _lib.ptr(bias), int(bool(relu)), int(cout),
                   _lib.ptr(out), out.shape[1], int(out_offset), _lib.stream()), name)
    return out


# largest map (input or output, bytes) the F(4x4, 3x3) kernel addresses: it stores with 32-bit byte offsets
# (lidar_wino43_conv3x3_nhwc refuses 2^31 - 1 and more).  A list so that tests can lower it.
_F43_MAX_BYTES = [2 ** 31 - 1]


def f43_fits(x_shape, cout, out=None):
    """the F(4x4, 3x3) kernel can serve conv3x3_auto(x, ..., cout, out=out) for an x of shape x_shape (B, Cin, H, W): input and
    output map both under _F43_MAX_BYTES, the output being `out` when given, else the (B, cout, H, W) map conv3x3_auto allocates.
    Pure host arithmetic (no library call)."""
    B, cin, H, W = (int(v) for v in x_shape)
    out_elems = out.numel() if out is not None else B * int(cout) * H * W
    return B * cin * H * W * 4 < _F43_MAX_BYTES[0] and out_elems * 4 < _F43_MAX_BYTES[0]


def kernel_for(cin, cout, x_shape=None, out=None):
    """which kernel runs a (Cin -> Cout) layer: "f43" (csrc/wino43_conv.hip) where LIDAR_WINO_F43 != 0, the kernel takes the widths
    and, for a map of shape x_shape (written into `out` when given), the map fits its 32-bit byte offsets (f43_fits); else "f23"
    (csrc/wino_conv.hip).  x_shape=None: the widths alone, before any map is known.  Pure host."""
    return "f43" if _F43[0] and supported43(cin, cout) and (x_shape is None or f43_fits(x_shape, cout, out)) else "f23"


def pack_auto(w):
    """-> [kind, packed filters, weight, F(2x2) filters]: the filters of kernel_for(Cin, Cout).  An "f43" entry carries the
    F(2x2, 3x3) filters too (16 Cin Cout more floats), packed here on the caller's stream: a map too large for the F(4x4) kernel's
    32-bit byte offsets (f43_fits) is served by F(2x2), and filters packed on first need would be written on whichever stream met
    that map first while another stream may already read them.  The F(4x4) filters are in the layout of the shared-transform
    workgroup shape (pack_weights43_share) where LIDAR_WINO43_SHARE != 0 and Cout % 128 == 0; conv3x3_auto reads the mark."""
    if kernel_for(w.shape[1], w.shape[0]) == "f43":
        share = _F43_SHARE[0] and supported43_share(w.shape[1], w.shape[0])
        return ["f43", pack_weights43_share(w) if share else pack_weights43(w), w.detach(), pack_weights(w)]
    return ["f23", pack_weights(w), None]


def conv3x3_auto(x, packed, cout, bias=None, relu=True, out=None, out_offset=0):
    """conv3x3 with the filters of pack_auto: the kernel kernel_for names for this map, among those the filters were packed for"""
    if packed[0] == "f43" and kernel_for(x.shape[1], cout, x.shape, out) == "f43":
        return conv3x3_f43(x, packed[1], cout, bias, relu, out, out_offset, share=getattr(packed[1], "w43_share", False))
    return conv3x3(x, packed[3 if packed[0] == "f43" else 1], cout, bias, relu, out, out_offset)   # ("f43" entry, oversize map: its F(2x2) filters)


def conv3x3_grouped_compact(x, packed, group_cin, couts, bias=None, relu=False, tables=None):
    """conv3x3_grouped with only the REAL output channels written: -> (B, sum(couts), H, W) channels-last, group g at channels
    [sum(couts[:g]), + couts[g]).  tables = (grp_cout, grp_ooff) device int32 tensors from a previous call (returned as second value)."""
    _lib.require_cuda(packed, bias)
    _lib.require_nhwc(x, "wino.conv3x3_grouped_compact")
    B, C, H, W = x.shape
    n = len(couts)
    L = _lib.lib()
    if n * group_cin > C or packed.numel() != L.lidar_wino_packed_floats(group_cin, 32 * n) or packed.numel() == 0 or max(couts) > 32 or min(couts) < 1:
        raise _lib.LidarHipError("wino.conv3x3_grouped_compact: groups / packed filters do not match the input")
    if bias is not None and bias.numel() != 32 * n:
        raise _lib.LidarHipError("wino.conv3x3_grouped_compact: bias must hold 32 * n_groups values (padded like the filters)")
    if tables is None:
        offs = [0]
        for c in couts[:-1]:
            offs.append(offs[-1] + int(c))
        tables = (torch.tensor([int(c) for c in couts], dtype=torch.int32, device=x.device), torch.tensor(offs, dtype=torch.int32, device=x.device))
    ctot = int(sum(couts))
    out, _ = _lib.nhwc_out("wino.conv3x3_grouped_compact", B, (H, W), ctot, x.device)
    _lib.check(L.lidar_wino_conv3x3_grouped_compact_nhwc(_lib.ptr(x), B, H, W, C, int(group_cin), n, _lib.ptr(packed), _lib.ptr(bias),
                                                         int(bool(relu)), _lib.ptr(tables[0]), _lib.ptr(tables[1]), _lib.ptr(out), ctot, 0,
                                                         _lib.stream()), "lidar_wino_conv3x3_grouped_compact_nhwc")
    return out, tables


def conv3x3_grouped(x, packed, group_cin, n_groups, bias=None, relu=False, out=None, out_offset=0):
    """n_groups independent 3x3 / padding-1 convolutions in one launch: group g reads channels [g * group_cin, (g + 1) * group_cin) of the
    channels-last x (B, C >= n_groups * group_cin, H, W) and writes channels [32 g, 32 g + 32) of the result (B, 32 n_groups, H, W).
    packed = pack_weights of the stacked (32 n_groups, group_cin, 3, 3) filters (groups with fewer outputs: zero rows)."""
    _lib.require_cuda(packed, bias)
    _lib.require_nhwc(x, "wino.conv3x3_grouped")
    B, C, H, W = x.shape
    cout = 32 * int(n_groups)
    L = _lib.lib()
    if n_groups * group_cin > C or packed.numel() != L.lidar_wino_packed_floats(group_cin, cout) or packed.numel() == 0:
        raise _lib.LidarHipError("wino.conv3x3_grouped: groups / packed filters do not match the input")
    if bias is not None and bias.numel() != cout:
        raise _lib.LidarHipError("wino.conv3x3_grouped: bias must hold 32 * n_groups values")
    out, out_offset = _lib.nhwc_out("wino.conv3x3_grouped", B, (H, W), cout, x.device, out, out_offset)
    _lib.check(L.lidar_wino_conv3x3_grouped_nhwc(_lib.ptr(x), B, H, W, C, int(group_cin), int(n_groups), _lib.ptr(packed), _lib.ptr(bias),
                                                 int(bool(relu)), _lib.ptr(out), out.shape[1], int(out_offset), _lib.stream()),
               "lidar_wino_conv3x3_grouped_nhwc")
    return out


# ------------------------------------------------------------------ weight gradient (csrc/wino43_wgrad.hip)
def wgrad43_supported(cin, cout):
    """the F(3x3, 4x4) weight-gradient kernel takes this layer: Cin and Cout multiples of 32 in [32, 512]"""
    return bool(_lib.lib().lidar_wino43_wgrad_supported(int(cin), int(cout)))


def wgrad43_fits(x_shape, cout, x_ld=None, g_ld=None):
    """the weight-gradient kernel can address an x of shape x_shape (B, Cin, H, W) and its (B, cout, H, W) output gradient: both
    maps (at their row strides x_ld / g_ld, default: the channel counts) under _F43_MAX_BYTES and not empty.  Pure host arithmetic
    (no library call)."""
    B, cin, H, W = (int(v) for v in x_shape)
    x_ld, g_ld = cin if x_ld is None else int(x_ld), int(cout) if g_ld is None else int(g_ld)
    return (B > 0 and H > 0 and W > 0 and B * H * W * x_ld * 4 < _F43_MAX_BYTES[0] and B * H * W * g_ld * 4 < _F43_MAX_BYTES[0])


def conv3x3_wgrad_f43(x, g):
    """the weight gradient of conv2d(x, w, stride=1, padding=1): x (B, Cin, H, W) and the output gradient g (B, Cout, H, W), both
    channels-last fp32 maps or channel slices of such maps -> dW (Cout, Cin, 3, 3) fp32, contiguous.  Winograd F(3x3, 4x4) on the
    matrix cores, partial sums over <= 512 tiles in fp32, the rest in fp64; bitwise reproducible; no host synchronisation."""
    from . import workspace
    x_ld, g_ld = _lib.nhwc_ld(x, "wino.conv3x3_wgrad_f43 x"), _lib.nhwc_ld(g, "wino.conv3x3_wgrad_f43 g")
    B, cin, H, W = x.shape
    cout = g.shape[1]
    if g.shape[0] != B or tuple(g.shape[2:]) != (H, W) or g.device != x.device:
        raise _lib.LidarHipError(f"wino.conv3x3_wgrad_f43: x {tuple(x.shape)} and g {tuple(g.shape)} must share batch, height, width and device")
    if not wgrad43_supported(cin, cout):
        raise _lib.LidarHipError(f"wino.conv3x3_wgrad_f43: (Cin, Cout) = ({cin}, {cout}) is not supported (multiples of 32 in [32, 512])")
    if not wgrad43_fits(x.shape, cout, x_ld, g_ld):
        raise _lib.LidarHipError(f"wino.conv3x3_wgrad_f43: maps of shape {tuple(x.shape)} / {tuple(g.shape)} are empty or too large (wgrad43_fits)")
    L = _lib.lib()
    wsb = L.lidar_wino43_wgrad_workspace_bytes(B, H, W, cin, cout)
    ws = workspace.get("wino43_wgrad", wsb, x.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    _lib.check(L.lidar_wino43_wgrad_nhwc(_lib.ptr(x), x_ld, _lib.ptr(g), g_ld, B, H, W, cin, cout, _lib.ptr(dw), _lib.ptr(ws), wsb,
                                         _lib.stream()), "lidar_wino43_wgrad_nhwc")
    return dw
