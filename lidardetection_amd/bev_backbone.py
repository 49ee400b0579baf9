"""Inference fast path of the dense BEV backbone + anchor head.

FoldedBEVBackbone evaluates the reference's BaseBEVBackbone + AnchorHeadSingle in eval mode, channels-last fp32:
  * eval-mode BatchNorm2d is folded into the preceding convolution (scale -> weights, shift -> bias) — the
    reference's Conv2d/BN/ReLU triplets (pcdet/models/backbones_2d/base_bev_backbone.py:34-45) and
    ConvTranspose2d/BN/ReLU deblocks (base_bev_backbone.py:51-57);
  * the first layer runs from the pillars as a sparse implicit GEMM when it can (csrc/pillar.hip), the stride-1 3x3 layers as
    Winograd F(4x4, 3x3) / F(2x2, 3x3) on the fp32 MFMA with shift + ReLU in the kernel (csrc/wino43_conv.hip, csrc/wino_conv.hip);
    the remaining (strided) convolutions stay stock torch (MIOpen) followed by ONE in-place shift + ReLU pass
    (`lidar_bias_act_nhwc`);
  * ConvTranspose2d deblocks with kernel == stride are GEMMs on the NHWC map that write their channel slice of the concatenated
    map (base_bev_backbone.py:103) directly, so `torch.cat` disappears: stride > 1 on csrc/deconv_gemm.hip (pixel shuffle in the
    epilogue), stride 1 as one hipBLASLt call with the map's row pitch (csrc/dense_gemm.hip);
  * a batch of 16 and more runs as two part-batches on two streams (_merged_split);
  * the three 1x1 heads of AnchorHeadSingle (pcdet/models/dense_heads/anchor_head_single.py:18-33,45-55) are one merged
    hipBLASLt GEMM on the concatenated map — or, for a caller that reads box and direction at selected anchors only
    (merged(defer=True)), the class columns alone, the rest computed later for just those anchors (DeferredHead,
    csrc/head_rows.hip).
Results match the unfolded modules to fp32 rounding (folding re-associates one multiply); tests assert 1e-4.
"""
import ctypes as C
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, wino, workspace


def bias_act_(x, bias, relu=True, out=None, out_offset=0):
    """x: (B, C, H, W) channels-last fp32.  out=None: in place.  Otherwise out is a channels-last (B, C_out, H, W)
    tensor and the result lands in channels [out_offset, out_offset + C)."""
    _lib.require_cuda(bias)
    if not (x.is_cuda and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        raise _lib.LidarHipError("bias_act_: expected a channels-last CUDA tensor")
    B, C, H, W = x.shape
    out, out_offset = (x, 0) if out is None else _lib.nhwc_out("bias_act_", B, (H, W), C, x.device, out, out_offset)
    _lib.check(_lib.lib().lidar_bias_act_nhwc(_lib.ptr(x), _lib.ptr(bias), B * H * W, C, int(bool(relu)), _lib.ptr(out),
                                              out.shape[1], int(out_offset), _lib.stream()), "lidar_bias_act_nhwc")
    return out


_LT_GEMM = [os.environ.get("LIDAR_BEV_LT_GEMM", "1") != "0"]      # the fused stride-1 deblock (csrc/dense_gemm.hip); A/B switch
_SPLIT_MIN = [int(os.environ.get("LIDAR_BEV_SPLIT_MIN", "8"))]    # fewest frames per part-batch
_SPLIT = [int(os.environ.get("LIDAR_BEV_SPLIT", "2"))]            # part-batches / streams of FoldedBEVBackbone.merged (1 = off)
_WINO = [os.environ.get("LIDAR_BEV_WINO", "1") != "0"]            # stride-1 3x3 layers on csrc/wino_conv.hip (0: MIOpen + epilogue pass)
_DECONV = [os.environ.get("LIDAR_BEV_DECONV", "1") != "0"]        # stride > 1 deblocks on csrc/deconv_gemm.hip (0: library GEMM + pixel-shuffle pass)
_SPARSE_FIRST = [os.environ.get("LIDAR_BEV_SPARSE_FIRST", "1") != "0"]   # first layer straight from the pillars (0: dense canvas + MIOpen)
_HEAD_DEFER = [os.environ.get("LIDAR_HEAD_DEFER", "1") != "0"]    # merged(defer=True): cls columns now, box / dir at the selected anchors later (0: all columns)


class DeferredHead:
    """What a cls-only head map (FoldedBEVBackbone.merged(defer=True)) needs to produce its box / direction columns later: the
    concat buffer(s) it was computed from (frame f in parts[f // frames_per_part]), the full head weight and bias with the column
    offsets of the box and direction heads, and the generation of every buffer at that time.  The buffers belong to the backbone and
    are overwritten by its next forward; rows() refuses to read them once that has happened."""

    def __init__(self, owner, slots, parts, head_wt, head_b, box_off, dir_off):
        self.owner, self.slots, self.parts = owner, tuple(slots), tuple(parts)
        self.gens = tuple(owner._cat_gen[s] for s in slots)
        self.head_wt, self.head_b, self.box_off, self.dir_off = head_wt, head_b, int(box_off), int(dir_off)
        self.frames_per_part = parts[0].shape[0]

    def stale(self):
        o = self.owner
        return any(o._cat_gen.get(s) != g or o._cats.get(s) is not p for s, g, p in zip(self.slots, self.gens, self.parts))

    def rows(self, anchors_per_loc, num_dir_bins, top_idx=None, who="DeferredHead.rows"):
        """-> logits (B, k, 7 + num_dir_bins) at the anchors top_idx (B, k) names, or at every anchor (anchor_post.head_rows)"""
        from . import anchor_post
        if self.stale():
            raise _lib.LidarHipError(f"{who}: this deferred head is stale — the backbone's concat buffers it reads its box / direction "
                                     "columns from were overwritten by a later forward (post-process a head before the next "
                                     "backbone_head call, or run with LIDAR_HEAD_DEFER=0)")
        return anchor_post.head_rows([p.permute(0, 2, 3, 1) for p in self.parts], self.head_wt, self.head_b, anchors_per_loc,
                                     self.box_off, self.dir_off, num_dir_bins, top_idx)


def _lt_gemm(a_ptr, M, K, w_kn, bias, relu, d_ptr, ldd, device):
    """D (M rows at pitch ldd) = act(A (M, K) @ w_kn (K, N) + bias): lidar_dense_gemm_bias_act (hipBLASLt, candidates timed once
    per shape).  False: the library path is not available (nothing written)."""
    ws = workspace.get("dense_gemm", 32 << 20, device)
    st = _lib.lib().lidar_dense_gemm_bias_act(a_ptr, M, K, _lib.ptr(w_kn), w_kn.shape[1], _lib.ptr(bias), int(bool(relu)), d_ptr, ldd,
                                              _lib.ptr(ws), ws.numel(), _lib.stream())
    if st == _lib.LIMITS["LIDAR_ERR_UNSUPPORTED"]:
        return False
    _lib.check(st, "lidar_dense_gemm_bias_act")
    return True


def _side_streams(device, n):
    """the n (<= 2) side streams of the split forward: the SAME two streams the sparse forward uses for its mask orders and rulebooks
    (spconv/conv.py, spconv/modules.py — never busy at the same time as a dense backbone).  A process drives only a few hardware
    queues (4 by default); streams beyond them share queues and serialise falsely: with each subsystem owning its own streams
    (7 in bench.py's `extra` process) the three-stream sparse forward measured there went from 3.15 to 4.4 ms."""
    from .spconv import conv as _sc, modules as _sm
    dev = torch.device(device)
    out = []
    for pool in (_sc._SIDE_STREAMS, _sm._RULEBOOK_STREAMS)[:n]:
        st = pool.get(dev)
        if st is None:
            st = pool[dev] = torch.cuda.Stream(dev, priority=-1)
        out.append(st)
    return out


def gemm_bias_act_into_(x, w_kn, bias, out, out_offset, relu=True):
    """x (B, K, h, w) channels-last, w_kn (K, N), bias (N): out[:, out_offset:out_offset+N] = act(x_rows @ w_kn + bias) with `out`
    (B, C_out, h, w) channels-last — one hipBLASLt GEMM whose epilogue writes at the map's row pitch.
    Returns False when the library path is not available (nothing written)."""
    _lib.require_cuda(w_kn, bias)
    _lib.require_nhwc(x, "gemm_bias_act_into_")
    B, K, h, w = x.shape
    N = w_kn.shape[1]
    if w_kn.shape[0] != K or bias.numel() != N:
        raise _lib.LidarHipError("gemm_bias_act_into_: shapes do not match")
    out, out_offset = _lib.nhwc_out("gemm_bias_act_into_", B, (h, w), N, x.device, out, out_offset)
    return _lt_gemm(_lib.ptr(x), B * h * w, K, w_kn, bias, relu, C.c_void_p(out.data_ptr() + 4 * out_offset), out.shape[1], x.device)


def rows_gemm(a2d, w_kn, bias=None, out=None):
    """a2d (M, K) @ w_kn (K, N) (+ bias) -> (M, N) (into `out`, contiguous, when given): the library GEMM with its candidates timed
    once per shape; torch.mm / addmm when that path is not available."""
    if _LT_GEMM[0] and a2d.is_cuda and a2d.dtype == torch.float32 and a2d.is_contiguous() and w_kn.is_contiguous():
        if out is None:
            out = torch.empty((a2d.shape[0], w_kn.shape[1]), dtype=torch.float32, device=a2d.device)
        elif not out.is_contiguous() or out.shape != (a2d.shape[0], w_kn.shape[1]):
            raise _lib.LidarHipError("rows_gemm: out must be a contiguous (M, N) tensor")
        if _lt_gemm(_lib.ptr(a2d), a2d.shape[0], a2d.shape[1], w_kn, bias, False, _lib.ptr(out), w_kn.shape[1], a2d.device):
            return out
        _LT_GEMM[0] = False
    if out is None:
        return torch.mm(a2d, w_kn) if bias is None else torch.addmm(bias, a2d, w_kn)
    return torch.mm(a2d, w_kn, out=out) if bias is None else torch.addmm(bias, a2d, w_kn, out=out)


def deconv_supported(K, s, c_up):
    return bool(_lib.lib().lidar_deconv_supported(int(K), int(s), int(c_up)))


def deconv_pack(w_kn):
    """(K, s*s*C_up) folded ConvTranspose2d weight, columns (ky, kx, c) -> packed form of csrc/deconv_gemm.hip"""
    _lib.require_cuda(w_kn)
    K, N = w_kn.shape
    L = _lib.lib()
    n = L.lidar_deconv_packed_floats(K, N)
    if n == 0:
        raise _lib.LidarHipError(f"deconv_pack: unsupported shape ({K}, {N})")
    packed = torch.empty(n, dtype=torch.float32, device=w_kn.device)
    _lib.check(L.lidar_deconv_pack_weights(_lib.ptr(w_kn.contiguous()), K, N, _lib.ptr(packed), _lib.stream()), "lidar_deconv_pack_weights")
    return packed


# largest map (input or output, bytes) csrc/deconv_gemm.hip addresses: it loads and stores with 32-bit byte offsets
# (lidar_deconv_gemm_nhwc refuses 2^31 - 1 and more).  A list so that tests can lower it.
_DECONV_MAX_BYTES = [2 ** 31 - 1]


def deconv_fits(B, K, h, w, s, out_c):
    """the fused deblock kernel can read the (B, K, h, w) map and write the (B, out_c, s*h, s*w) concat map; else the two-step path"""
    return B * h * w * K * 4 < _DECONV_MAX_BYTES[0] and B * h * w * s * s * out_c * 4 < _DECONV_MAX_BYTES[0]


def deconv_gemm_into_(x, packed, bias, s, out, out_offset=0, relu=True):
    """x (B, K, h, w) channels-last -> out[:, out_offset:out_offset + C_up] (B, C_out, s*h, s*w channels-last) = act(ConvTranspose2d
    (kernel == stride == s)(x) + bias): one fp32-MFMA kernel, no temporary, no pixel-shuffle pass (csrc/deconv_gemm.hip)"""
    _lib.require_cuda(packed, bias)
    _lib.require_nhwc(x, "deconv_gemm_into_")
    B, K, h, w = x.shape
    c_up = bias.numel()
    if packed.numel() != K * s * s * c_up:
        raise _lib.LidarHipError("deconv_gemm_into_: packed weights do not match (K, s, C_up)")
    out, out_offset = _lib.nhwc_out("deconv_gemm_into_", B, (s * h, s * w), c_up, x.device, out, out_offset)
    _lib.check(_lib.lib().lidar_deconv_gemm_nhwc(_lib.ptr(x), B, h, w, K, _lib.ptr(packed), _lib.ptr(bias), int(bool(relu)), int(s), c_up,
                                                 _lib.ptr(out), out.shape[1], int(out_offset), _lib.stream()), "lidar_deconv_gemm_nhwc")
    return out


def bias_act_upsample_(y2d, bias, batch, h, w, s, out, out_offset=0, relu=True):
    """y2d: (batch*h*w, s*s*C) GEMM output of a kernel==stride transposed conv, columns ordered (ky, kx, c).
    Writes act(y + bias) pixel-shuffled into channels [out_offset, out_offset + C) of the channels-last `out`."""
    _lib.require_cuda(y2d, bias)
    C = bias.numel()
    if y2d.shape != (batch * h * w, s * s * C):
        raise _lib.LidarHipError("bias_act_upsample_: GEMM output shape does not match (batch*h*w, s*s*C)")
    out, out_offset = _lib.nhwc_out("bias_act_upsample_", batch, (h * s, w * s), C, y2d.device, out, out_offset)
    _lib.check(_lib.lib().lidar_bias_act_upsample_nhwc(_lib.ptr(y2d), _lib.ptr(bias), batch, h, w, s, C, int(bool(relu)),
                                                       _lib.ptr(out), out.shape[1], int(out_offset), _lib.stream()),
               "lidar_bias_act_upsample_nhwc")
    return out


def collect_params(*modules):
    """every parameter and buffer of `modules` (collected once: the module tree does not change)"""
    out = []
    for m in modules:
        out += list(m.parameters()) + list(m.buffers())
    return out


def params_key(tensors):
    """identity + version of the source tensors: changes whenever load_state_dict(), .to(), an optimizer step or a
    BatchNorm statistics update touches one of them (same idea as SparseConvolution._folded)"""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def _fold(weight, bn, out_dim, conv_bias=None):
    """scale the conv weight along its output-channel dim by gamma/sqrt(var+eps); return (weight, shift).
    A convolution bias (the reference uses bias=False) is folded as bias*scale + shift."""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias.detach() - bn.running_mean * scale
    if conv_bias is not None:
        shift = shift + conv_bias.detach() * scale
    shape = [1] * weight.dim()
    shape[out_dim] = -1
    return (weight.detach() * scale.view(shape)), shift.contiguous()


class BlockLayer(NamedTuple):
    """One [ZeroPad2d] Conv2d BatchNorm2d ReLU group of a block (parse_block): the modules and the padding they add up to.  The
    folded inference path (FoldedBEVBackbone) and the train path (bev_train) both route from this record."""
    zpad: Optional[nn.ZeroPad2d]
    conv: nn.Conv2d
    bn: nn.BatchNorm2d
    act: Optional[nn.ReLU]
    pad: Optional[tuple]              # the conv's zero padding (h, w) with a symmetric ZeroPad2d folded in (no padded copy); None: string padding / another padding mode
    zero_pad: Optional[tuple]         # (left, right, top, bottom) of a ZeroPad2d that is not folded and stays a separate F.pad, else None

    @property
    def plain3x3(self):
        """stride 1, 3x3, zero padding 1 and nothing else: the geometry the Winograd kernels compute (LAYER_NUMS per block,
        base_bev_backbone.py:40-45; SECOND's first block opens with one too).  The widths: wino.supported / wino_train_supported."""
        c = self.conv
        return (self.pad == (1, 1) and self.zero_pad is None and tuple(c.kernel_size) == (3, 3) and tuple(c.stride) == (1, 1)
                and tuple(c.dilation) == (1, 1) and c.groups == 1)


def block_layer(zpad, conv, bn, act=None):
    """-> the BlockLayer of ZeroPad2d `zpad` (or None), Conv2d, BatchNorm2d, ReLU.  Pure host."""
    pad, zero_pad = None, None if zpad is None else tuple(int(v) for v in zpad.padding)
    if conv.padding_mode == "zeros" and not isinstance(conv.padding, str):
        pad = tuple(int(v) for v in conv.padding)
        if zero_pad is not None and zero_pad[0] == zero_pad[1] >= 0 and zero_pad[2] == zero_pad[3] >= 0:
            pad, zero_pad = (pad[0] + zero_pad[2], pad[1] + zero_pad[0]), None
    return BlockLayer(zpad, conv, bn, act, pad, zero_pad)


def parse_block(blk):
    """Sequential of [ZeroPad2d] Conv2d BatchNorm2d ReLU ... -> [BlockLayer], or None for any other structure"""
    mods, out, i = list(blk), [], 0
    while i < len(mods):
        zpad = None
        if isinstance(mods[i], nn.ZeroPad2d):
            zpad, i = mods[i], i + 1
        if i + 3 > len(mods):
            return None
        conv, bn, act = mods[i:i + 3]
        if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d) and isinstance(act, nn.ReLU)):
            return None
        out.append(block_layer(zpad, conv, bn, act))
        i += 3
    return out


class FoldedConv(NamedTuple):
    """one folded Conv2d/BN/ReLU layer of a stage"""
    weight: torch.Tensor              # BatchNorm scale folded in, channels-last
    shift: torch.Tensor
    stride: tuple
    pad: tuple                        # BlockLayer.pad
    dilation: tuple
    groups: int
    zero_pad: Optional[tuple]         # BlockLayer.zero_pad
    wino: Optional[list]              # wino.pack_auto's filters for a layer on the Winograd kernels, else None


class FoldedDeblock(NamedTuple):
    """the folded deblock of a stage.  kind: "gemm" (ConvTranspose2d with kernel == stride: a plain GEMM on the NHWC map),
    "deconv_mfma" (the same on csrc/deconv_gemm.hip), "deconv" / "conv" (any other ConvTranspose2d / a strided Conv2d: the library)"""
    kind: str
    weight: torch.Tensor              # "gemm" / "deconv_mfma": (K, s*s*C_up), columns (ky, kx, c); else the module's, channels-last
    packed: Optional[torch.Tensor]    # "deconv_mfma": deconv_pack(weight)
    shift: torch.Tensor
    stride: int                       # "gemm" / "deconv_mfma": s (0 for the library kinds)
    args: tuple                       # "deconv" / "conv": what F.conv_transpose2d / F.conv2d take after the bias (() for the others)


def _cl(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


class FoldedBEVBackbone:
    """Built from the (eval-mode) reference-shaped modules; call with the channels-last canvas.  self.stages: one
    ([FoldedConv], FoldedDeblock) per block."""

    def __init__(self, blocks, deblocks, heads):
        self.sources = collect_params(blocks, deblocks, *heads)
        self.source_key = params_key(self.sources)                  # owners rebuild when this no longer matches
        self.stages = []
        for blk, de in zip(blocks, deblocks):
            layers = parse_block(blk)
            assert layers is not None, "FoldedBEVBackbone: blocks must be [ZeroPad2d] Conv2d BatchNorm2d ReLU groups"
            convs = []
            for l in layers:
                assert l.pad is not None, "FoldedBEVBackbone: explicit zero padding only"
                w, b = _fold(l.conv.weight, l.bn, 0, l.conv.bias)
                packed = None
                if _WINO[0] and w.is_cuda and l.plain3x3 and wino.supported(w.shape[1], w.shape[0]):
                    packed = wino.pack_auto(w)        # Winograd on the matrix cores, shift + ReLU in the kernel (csrc/wino43_conv.hip, csrc/wino_conv.hip)
                convs.append(FoldedConv(w.contiguous(memory_format=torch.channels_last), b, tuple(l.conv.stride), l.pad,
                                        tuple(l.conv.dilation), l.conv.groups, l.zero_pad, packed))
            up, bn = de[0], de[1]
            assert tuple(up.dilation) == (1, 1) and up.groups == 1 and up.padding_mode == "zeros", \
                "FoldedBEVBackbone: deblocks with dilation, groups or non-zero padding modes are not supported"
            if isinstance(up, nn.ConvTranspose2d):
                w, b = _fold(up.weight, bn, 1, up.bias)
                s = up.stride[0]
                if tuple(up.kernel_size) == tuple(up.stride) and s == up.stride[1] and \
                        tuple(up.padding) == (0, 0) and tuple(up.output_padding) == (0, 0):
                    # kernel == stride: every input pixel owns its own s x s output patch -> a plain GEMM
                    w_kn = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()
                    upc = FoldedDeblock("gemm", w_kn, None, b, s, ())
                    if _DECONV[0] and w.is_cuda and s > 1 and deconv_supported(w_kn.shape[0], s, b.numel()):
                        upc = upc._replace(kind="deconv_mfma", packed=deconv_pack(w_kn))   # csrc/deconv_gemm.hip (maps of 2 GiB and more: the plain weight)
                else:
                    upc = FoldedDeblock("deconv", w.contiguous(memory_format=torch.channels_last), None, b, 0,
                                        (up.stride, up.padding, up.output_padding))
            else:   # stride < 1 in the reference config: a strided Conv2d (base_bev_backbone.py:60-69)
                w, b = _fold(up.weight, bn, 0, up.bias)
                upc = FoldedDeblock("conv", w.contiguous(memory_format=torch.channels_last), None, b, 0, (up.stride, up.padding))
            self.stages.append((convs, upc))
        self.up_channels = [up.shift.numel() for _, up in self.stages]
        for h in heads:
            assert tuple(h.kernel_size) == (1, 1) and tuple(h.stride) == (1, 1)
        self.head_split = [h.weight.shape[0] for h in heads]
        if heads:   # (a backbone used without merged 1x1 heads — e.g. AnchorHeadMulti's 3x3 branches — calls features() only)
            self.head_wt = torch.cat([h.weight.detach().flatten(1) for h in heads], 0).t().contiguous()   # (C_in, sum C_head)
            self.head_b = torch.cat([h.bias.detach() if h.bias is not None else h.weight.new_zeros(h.weight.shape[0])
                                     for h in heads], 0).contiguous()
            # the first head alone (cls when the heads are given as [cls, box, dir]): what merged(defer=True) computes for every row
            self.head0_wt = self.head_wt[:, :self.head_split[0]].contiguous()
            self.head0_b = self.head_b[:self.head_split[0]].contiguous()
        self._cats = {}                    # concat buffers, one per (slot of a split forward, shape)
        self._cat_gen = {}                 # slot -> how often features() has (re)written that buffer (DeferredHead.stale)
        self._streams = None
        # the first layer as a sparse implicit GEMM over the pillars (csrc/pillar.hip lidar_pillar_conv_table): (k*k, Cin, Cout) weights
        self._first_sparse = None
        c0 = self.stages[0][0][0]
        w0, b0, st0, pad0 = c0.weight, c0.shift, c0.stride, c0.pad
        k0 = w0.shape[2]
        if (w0.is_cuda and w0.shape[2] == w0.shape[3] and st0[0] == st0[1] and pad0[0] == pad0[1] and k0 * k0 <= 31
                and c0.dilation == (1, 1) and c0.groups == 1 and c0.zero_pad is None):   # (the neighbour table knows one stride and one symmetric pad)
            from .spconv import ops as _sops
            if _sops.sorted_gemm_supported(k0 * k0, w0.shape[1], w0.shape[0]):
                self._first_sparse = (w0.permute(2, 3, 1, 0).reshape(k0 * k0, w0.shape[1], w0.shape[0]).contiguous(), b0, k0, int(st0[0]), int(pad0[0]))

    def first_layer_from_pillars(self, pm):
        """pm: pillar_ops.PillarMap -> act(conv0(scatter(pm)) + shift) as a channels-last (B, Cout, OH, OW) map WITHOUT building the
        canvas: neighbour table over all output pixels (one tiny launch) + the mask-ordered sparse implicit GEMM, which writes every
        output pixel once (pixels no pillar reaches get act(shift)).  PointPillar-KITTI bs 16: 4.7 GFLOP instead of 63."""
        from . import pillar_ops
        from .spconv import ops as _sops
        w9, b0, k0, st0, pad0 = self._first_sparse
        nbr, OH, OW = pillar_ops.pillar_conv_table(pm.coords, pm.B, pm.nx, pm.ny, k0, st0, pad0, pm.num_voxels_dev)
        order = _sops.mask_order(nbr)
        out = _sops.indice_conv_fused(pm.features, nbr, w9, b0, None, True, order)           # (B * OH * OW, Cout) = the NHWC map
        return out.view(pm.B, OH, OW, w9.shape[2]).permute(0, 3, 1, 2)

    def sparse_first_ok(self):
        return self._first_sparse is not None and _SPARSE_FIRST[0]

    def features(self, canvas, slot=0, first_done=False):
        """-> the concatenated upsampled map (B, sum(up_channels), H, W), channels-last.  first_done: `canvas` is already the output
        of the first layer (first_layer_from_pillars)."""
        x, cat, off = canvas, None, 0
        for si, (convs, up) in enumerate(self.stages):
            for ci, cv in enumerate(convs):
                if first_done and si == 0 and ci == 0:
                    continue
                if cv.wino is not None and _WINO[0] and x.is_contiguous(memory_format=torch.channels_last):
                    x = wino.conv3x3_auto(x, cv.wino, cv.weight.shape[0], cv.shift, True)
                    continue
                if cv.zero_pad is not None:
                    x = F.pad(x, cv.zero_pad)
                x = _cl(F.conv2d(x, cv.weight, None, cv.stride, cv.pad, cv.dilation, cv.groups))
                bias_act_(x, cv.shift)
            B, _, h, w = x.shape
            y = None
            if up.kind in ("deconv", "conv"):            # the library convolution; its epilogue follows once the concat map exists
                y = _cl((F.conv_transpose2d if up.kind == "deconv" else F.conv2d)(x, up.weight, None, *up.args))
            oh, ow = (h * up.stride, w * up.stride) if y is None else y.shape[2:]
            if cat is None:
                shape = (B, sum(self.up_channels), oh, ow)
                cat = self._cats.get(slot)
                if cat is None or cat.shape != shape or cat.device != x.device:
                    cat = self._cats[slot] = torch.empty(shape, dtype=torch.float32, device=x.device,
                                                         memory_format=torch.channels_last)
                self._cat_gen[slot] = self._cat_gen.get(slot, 0) + 1      # about to be overwritten: deferred heads reading it are stale
            if y is not None:
                bias_act_(y, up.shift, out=cat, out_offset=off)
            else:
                self._deblock_gemm(x, up, cat, off)
            off += up.shift.numel()
        return cat

    def _deblock_gemm(self, x, up, cat, off):
        """a kernel == stride deblock into its channel slice of `cat`, on the first route that applies"""
        B, K, h, w = x.shape
        if up.kind == "deconv_mfma" and deconv_fits(B, K, h, w, up.stride, cat.shape[1]):
            return deconv_gemm_into_(x, up.packed, up.shift, up.stride, cat, off)                 # one fused kernel
        if up.kind == "gemm" and up.stride == 1 and _LT_GEMM[0]:
            # stride 1: GEMM + shift + ReLU + concat in ONE hipBLASLt call writing with the map's row pitch
            if gemm_bias_act_into_(x, up.weight, up.shift, cat, off):
                return cat
            _LT_GEMM[0] = False                                                                   # not available here: the two-step path from now on
        y = rows_gemm(x.permute(0, 2, 3, 1).reshape(B * h * w, -1), up.weight)                    # the NHWC map IS the row-major A
        return bias_act_upsample_(y, up.shift, B, h, w, up.stride, cat, off)                      # + shift, ReLU, pixel shuffle

    def stale(self):
        return params_key(self.sources) != self.source_key

    def _defer_ok(self, cat_bytes):
        """merged(defer=True) can defer: the switch is on, there is something after the first head to defer, and lidar_head_rows
        takes this channel count and part size (the anchor layout is the caller's to check: anchor_post.head_rows_supported)"""
        from . import anchor_post
        return (_HEAD_DEFER[0] and len(self.head_split) > 1 and self.head_wt.is_cuda
                and anchor_post.head_rows_supported(self.head_wt.shape[0], 1, 0, cat_bytes))

    def merged(self, canvas, defer=False):
        """-> the merged head output (B, H, W, sum C_head), channels [cls | box | dir] as the heads were given.
        canvas: the channels-last BEV map, or a pillar_ops.PillarMap (the first layer then runs from the pillars when it can).
        defer=True (for a caller that reads the later heads at selected anchors only, and passes the heads as [cls, box, dir]):
        only the FIRST head's columns are computed, (B, H, W, C_head[0]), and the returned tensor carries a DeferredHead as its
        plain attribute `deferred`, from which the other columns are computed at the anchors that need them
        (DeferredHead.rows).  That record reads this backbone's concat buffers: it is valid until the next forward of this
        backbone, and stale (an error, never the new batch's values) afterwards.  With LIDAR_HEAD_DEFER=0, or where
        lidar_head_rows does not support the shape, defer=True returns the full head like defer=False."""
        first_done = False
        if not torch.is_tensor(canvas):
            if self.sparse_first_ok():
                canvas, first_done = self.first_layer_from_pillars(canvas), True
            else:
                canvas = canvas.dense()
        B = canvas.shape[0]
        if 1 < _SPLIT[0] <= 2 and canvas.is_cuda and B % _SPLIT[0] == 0 and B // _SPLIT[0] >= _SPLIT_MIN[0]:   # (4-frame parts lost in r03: PV-RCNN bs 8 16.0 -> 17.5 ms)
            return self._merged_split(canvas, _SPLIT[0], first_done, defer)
        cat = self.features(canvas, first_done=first_done)
        B, C, H, W = cat.shape
        defer = bool(defer) and self._defer_ok(cat.numel() * 4)
        wt, b = (self.head0_wt, self.head0_b) if defer else (self.head_wt, self.head_b)
        out = rows_gemm(cat.permute(0, 2, 3, 1).reshape(B * H * W, C), wt, b).view(B, H, W, -1)       # 1x1 heads = one GEMM
        if defer:
            out.deferred = DeferredHead(self, (0,), (cat,), self.head_wt, self.head_b, self.head_split[0], sum(self.head_split[:2]))
        return out

    def _merged_split(self, canvas, n, first_done=False, defer=False):
        """The same forward as n part-batches on n streams: the convolutions are bound by the matrix cores (0.8 of the fp32 MFMA peak,
        < 0.5 TB/s of HBM traffic) and everything around them — MIOpen's zero-fill of each output, the shift + ReLU pass, the pixel
        shuffles — by HBM, and within one batch they are strictly serial; two part-batches let one's passes run under the other's
        convolutions (PointPillar bs 16: backbone + heads 9.94 -> 9.48 ms, step 10.52 -> 10.18 ms; SECOND bs 16: 18.49 -> 17.81 ms;
        8 frames alone cost 5.08 ms).  Same layers, same weights;
        the library may pick other kernels for the smaller batch, so results can differ from the whole-batch forward in the last bits."""
        dev = canvas.device
        cur = torch.cuda.current_stream(dev)
        self._streams = _side_streams(dev, n)
        B, hb = canvas.shape[0], canvas.shape[0] // n
        out, cats, wt, b = None, [], self.head_wt, self.head_b
        for i, st in enumerate(self._streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                cat = self.features(canvas[i * hb:(i + 1) * hb], slot=i + 1, first_done=first_done)
                cats.append(cat)
                _, C, H, W = cat.shape
                if out is None:
                    defer = bool(defer) and self._defer_ok(cat.numel() * 4)
                    if defer:
                        wt, b = self.head0_wt, self.head0_b
                    with torch.cuda.stream(cur):                       # owned by the caller's stream, written by the side streams
                        out = torch.empty((B, H, W, wt.shape[1]), dtype=torch.float32, device=dev)
                    st.wait_stream(cur)
                out.record_stream(st)
                rows_gemm(cat.permute(0, 2, 3, 1).reshape(hb * H * W, C), wt, b, out=out[i * hb:(i + 1) * hb].view(hb * H * W, -1))
        for st in self._streams:
            cur.wait_stream(st)
        if defer:
            out.deferred = DeferredHead(self, range(1, n + 1), cats, self.head_wt, self.head_b, self.head_split[0], sum(self.head_split[:2]))
        return out

    def __call__(self, canvas):
        """-> per-head maps in (B, H, W, C_head) layout (views of the merged head output)."""
        return torch.split(self.merged(canvas), self.head_split, dim=-1)
