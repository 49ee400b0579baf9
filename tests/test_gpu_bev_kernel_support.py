"""GPU checks of the dense inference BEV kernels over the ranges include/lidar_hip.h declares, each against a plain float64 reference
of the same operation on the CPU: csrc/deconv_gemm.hip (fused deblock), csrc/wino_conv.hip (Winograd F(2x2, 3x3), plain / grouped /
grouped-compact), csrc/wino43_conv.hip (F(4x4, 3x3)), csrc/dense_epilogue.hip and the csrc/dense_gemm.hip wrapper.  The other files
test these kernels at production-like points; here are the channel counts between them, the degenerate maps, the persistent walk
(more tile blocks than workgroups, so that every workgroup streams a NEXT block's input while it finishes the current one) and
real maps at the 32-bit byte limits.

Every input is drawn on the CPU from a seeded generator.  The one deliberate exception are the maps of section (d), all of them and
not only the 2 GiB one: at 1 .. 2 GiB each they come from a seeded generator on the device (every frame different, which a tiled
CPU-drawn frame would not give), so that a (d) test stays within seconds; their filters and biases are still drawn on the CPU.
Tolerance everywhere: err <= 1e-4 * max(1, |want|.max()), as in test_gpu_wino.py and test_gpu_deconv.py.  An output that is a slice
of a wider map is written into a map pre-filled with SENTINEL, and every channel outside the slice must still hold it bit for bit.
tests/test_bev_kernel_args_host.py checks the outside of the same ranges on the CPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from _gpu_util import release_memory  # noqa: F401  (release_memory: an autouse fixture)
from lidardetection_amd import _lib, wino
from lidardetection_amd import bev_backbone as bb
from test_bev_kernel_args_host import DECONV_LIMIT, F43_IN_LIMIT, F43_OUT_LIMIT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 777.0
BAR = 1e-4
CL = torch.channels_last


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _divup(a, b):
    return -(-a // b)


def _check(got, want, what):
    """got: device fp32, want: CPU float64 -> error relative to the scale; asserts the project's bar"""
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double() - want.to(got.device)).abs().max())
    print(f"{what}: max err {err:.2e} scale {scale:.1f} rel {err / scale:.2e}")
    assert err <= BAR * scale, (what, err, scale)
    return err / scale


def _sentinel_map(B, C_, H, W):
    return torch.full((B, C_, H, W), SENTINEL, device=DEV).contiguous(memory_format=CL)


def _outside_untouched(out, off, c):
    return bool((out[:, :off] == SENTINEL).all()) and bool((out[:, off + c:] == SENTINEL).all())


# ------------------------------------------------------------------ (a) the deblock kernel (csrc/deconv_gemm.hip)
def deconv_blocks(B, h, w, s, c_up):
    """n_blocks = divup(P, 128) * (s * s * C_up / 512)      csrc/deconv_gemm.hip:281-283 (the grid is capped at the CU count: :286-288)"""
    return _divup(B * h * w, 128) * (s * s * c_up // 512)


def _deconv_inputs(B, K, h, w, s, c_up, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, K, h, w, generator=g)
    wt = torch.randn(K, c_up, s, s, generator=g) / math.sqrt(K)       # ConvTranspose2d weight layout (Cin, Cout, kH, kW)
    bias = torch.randn(c_up, generator=g)
    return x, wt, bias


def _deconv_run(xd, packed, bias_d, relu, s, c_up, out, off, raw):
    B, K, h, w = xd.shape
    if raw:                                                          # straight through the C ABI: the only way to pass bias = NULL
        _lib.check(_lib.lib().lidar_deconv_gemm_nhwc(_lib.ptr(xd), B, h, w, K, _lib.ptr(packed), _lib.ptr(bias_d), int(relu), s, c_up,
                                                     _lib.ptr(out), out.shape[1], off, _lib.stream()), "lidar_deconv_gemm_nhwc")
    else:
        bb.deconv_gemm_into_(xd, packed, bias_d, s, out, off, relu)


def _deconv_case(B, K, h, w, s, c_up, out_c, off, relus=(True, False), no_bias=False, what="deconv"):
    assert bb.deconv_supported(K, s, c_up) and off % 4 == 0
    x, wt, bias = _deconv_inputs(B, K, h, w, s, c_up, 1000 * K + 10 * s + c_up + h + w)
    w_kn = wt.permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(DEV)            # columns (ky, kx, c)
    packed = bb.deconv_pack(w_kn)
    xd = x.to(DEV).contiguous(memory_format=CL)
    pre = F.conv_transpose2d(x.double(), wt.double(), None if no_bias else bias.double(), stride=s)
    worst = 0.0
    for relu in relus:
        out = _sentinel_map(B, out_c, s * h, s * w)
        _deconv_run(xd, packed, None if no_bias else bias.to(DEV), relu, s, c_up, out, off, raw=no_bias)
        worst = max(worst, _check(out[:, off:off + c_up], torch.relu(pre) if relu else pre, f"{what} {(B, K, h, w, s, c_up, out_c, off, relu)}"))
        assert _outside_untouched(out, off, c_up)
    return worst


# K in {16, 24, 40, 64, 256}, s in {1, 2, 3, 4, 8}, C_up in {128, 256, 384, 512}, the corners (K = 16, s = 8) and (K = 24, C_up = 384,
# s = 2); few blocks each (at most 16: never more blocks than workgroups), P % 128 != 0
DECONV_SWEEP = [
    (2, 16, 3, 5, 8, 128, 136, 4),           # 16 column groups of one pixel block
    (1, 24, 9, 11, 2, 384, 392, 4),          # C_up not a power of two: a 512-column group spans two (ky, kx); 3 chunk pairs
    (3, 40, 5, 7, 1, 512, 520, 8),           # s = 1; 5 chunk pairs
    (1, 64, 6, 5, 3, 512, 516, 4),           # s = 3: 9 groups
    (2, 256, 7, 9, 4, 256, 264, 4),
    (1, 40, 13, 11, 2, 256, 268, 12),        # two pixel blocks x two groups
    (1, 24, 10, 13, 4, 128, 140, 12),        # P = 130: a last block of two pixels
    (1, 16, 4, 4, 2, 384, 384, 0),           # the slice is the whole map
]


@pytest.mark.parametrize("B,K,h,w,s,c_up,out_c,off", DECONV_SWEEP)
def test_deconv_sweep_vs_float64(dev, B, K, h, w, s, c_up, out_c, off):
    assert deconv_blocks(B, h, w, s, c_up) <= 16
    _deconv_case(B, K, h, w, s, c_up, out_c, off)


@pytest.mark.parametrize("B,K,h,w,s,c_up,out_c,off", [DECONV_SWEEP[0], DECONV_SWEEP[1], DECONV_SWEEP[3]])
def test_deconv_without_bias_through_the_c_abi(dev, B, K, h, w, s, c_up, out_c, off):
    _deconv_case(B, K, h, w, s, c_up, out_c, off, no_bias=True, what="deconv bias=NULL")


# more blocks than workgroups at the fewest chunks per block (K = 16: 4, K = 24: 6): the A stream crosses into the NEXT block two
# chunks before the current block ends.  (B, K, h, w, relu): P odd, P % 128 in {1, 127}
DECONV_WALK = [(1, 16, 131, 171, True), (1, 24, 115, 197, False), (3, 16, 57, 131, False)]


@pytest.mark.parametrize("B,K,h,w,relu", DECONV_WALK)
def test_deconv_persistent_walk_vs_float64(dev, B, K, h, w, relu):
    s, c_up = 4, 128
    P, nblk = B * h * w, deconv_blocks(B, h, w, s, c_up)
    assert P % 2 == 1 and P % 128 in (1, 127)
    assert nblk >= 2.5 * _cus(), (nblk, _cus())                      # every workgroup walks two or more blocks
    _deconv_case(B, K, h, w, s, c_up, 132, 4, relus=(relu,), what="deconv walk")


def test_deconv_persistent_walk_is_deterministic(dev):
    B, K, h, w, s, c_up = 1, 24, 115, 197, 4, 128
    assert deconv_blocks(B, h, w, s, c_up) >= 2.5 * _cus()
    x, wt, bias = _deconv_inputs(B, K, h, w, s, c_up, 5)
    packed = bb.deconv_pack(wt.permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(DEV))
    xd, bd = x.to(DEV).contiguous(memory_format=CL), bias.to(DEV)
    a, b = _sentinel_map(B, 132, s * h, s * w), _sentinel_map(B, 132, s * h, s * w)
    bb.deconv_gemm_into_(xd, packed, bd, s, a, 4)
    bb.deconv_gemm_into_(xd, packed, bd, s, b, 4)
    assert torch.equal(a, b)


# the epilogue steps "two pixels on" with carries x -> y -> frame: maps where one step crosses a row AND a frame
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("B,h,w", [(300, 1, 1), (40, 1, 7), (40, 7, 1), (3, 2, 1), (129, 1, 1)])
def test_deconv_carry_edges_vs_float64(dev, B, h, w, s):
    _deconv_case(B, 16, h, w, s, 128, 136, 8, what="deconv carry")


# ------------------------------------------------------------------ (b) F(2x2, 3x3) (csrc/wino_conv.hip)
def f23_blocks(B, H, W, cout, grouped=False):
    """-> (n_blocks, tall, NW) as wino_launch decides them      csrc/wino_conv.hip:721-729:
    NW = grouped ? 1 : Cout % 128 == 0 ? 4 : Cout % 64 == 0 ? 2 : 1, MW = 4 / NW; tiles of 2 x 2 pixels;
    wide = divup(tiles_y, 4 MW) * divup(tiles_x, 8), tall = divup(tiles_y, 8 MW) * divup(tiles_x, 4), tall taken when smaller;
    n_blocks = B * blocks_y * blocks_x * (Cout / (32 NW))"""
    nw = 1 if grouped else 4 if cout % 128 == 0 else 2 if cout % 64 == 0 else 1
    mw = 4 // nw
    ty, tx = (H + 1) // 2, (W + 1) // 2
    wide, tall = _divup(ty, 4 * mw) * _divup(tx, 8), _divup(ty, 8 * mw) * _divup(tx, 4)
    return B * min(wide, tall) * (cout // (32 * nw)), tall < wide, nw


def _conv_inputs(B, in_c, cin, cout, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, in_c, H, W, generator=g)
    x[:, :, 0, :] += 2.0                                              # make the borders matter (zero padding must really be zero)
    x[:, :, :, -1] -= 3.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g)
    return x, w, bias


def _conv_ref(x, w, bias):
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 1, 1)


def _f23_case(B, cin, cout, H, W, variants, off=4, extra=8, what="f23"):
    """variants: (relu, with bias) pairs; the result goes into channels [off, off + cout) of a map of cout + extra channels"""
    x, w, bias = _conv_inputs(B, cin, cin, cout, H, W, 1000 * cin + cout + 7 * H + W)
    xd, packed, bd = x.to(DEV).contiguous(memory_format=CL), wino.pack_weights(w.to(DEV)), bias.to(DEV)
    pre = {True: _conv_ref(x, w, bias)}
    if any(not wb for _, wb in variants):
        pre[False] = pre[True] - bias.double().view(1, -1, 1, 1)     # the same float64 convolution without the shift
    worst = 0.0
    for relu, wb in variants:
        want = torch.relu(pre[wb]) if relu else pre[wb]
        out = _sentinel_map(B, cout + extra, H, W)
        wino.conv3x3(xd, packed, cout, bd if wb else None, relu, out=out, out_offset=off)
        worst = max(worst, _check(out[:, off:off + cout], want, f"{what} {(B, cin, cout, H, W, relu, wb)}"))
        assert _outside_untouched(out, off, cout)
    return worst


ALL3 = ((True, True), (False, False), (False, True))
# Cin in {16, 24, 40, 64} x Cout in {32, 96, 160 (NW = 1), 192 (NW = 2), 128 (NW = 4)}; (B, cin, cout, H, W, tall)
F23_SWEEP = [
    (1, 16, 32, 1, 1, False), (2, 24, 96, 1, 9, False), (1, 40, 160, 9, 1, False), (2, 64, 192, 2, 2, False), (1, 24, 128, 3, 5, False),
    (1, 40, 32, 40, 8, True),          # NW = 1 tall (64 x 8 pixels per block)
    (1, 64, 96, 20, 36, False),        # NW = 1 wide, three blocks x three channel groups
    (2, 16, 192, 32, 8, True),         # NW = 2 tall
    (1, 40, 192, 14, 36, False),       # NW = 2 wide
    (1, 24, 128, 16, 8, True),         # NW = 4 tall
    (2, 16, 128, 7, 37, False),        # NW = 4 wide
    (1, 24, 160, 33, 7, True),         # five channel groups, six chunks
    (1, 40, 96, 17, 19, False),
    (1, 16, 160, 5, 3, False),
]


@pytest.mark.parametrize("B,cin,cout,H,W,tall", F23_SWEEP)
def test_f23_sweep_vs_float64(dev, B, cin, cout, H, W, tall):
    assert f23_blocks(B, H, W, cout)[1] == tall
    _f23_case(B, cin, cout, H, W, ALL3)


# the input DMA runs three chunks ahead, across tile blocks, at the fewest chunks a block may hold (Cin = 16: 4; 24: 6), over
# frames (B >= 2), H and W no multiples of a block's 32 x 16 / 64 x 8 pixels.  (B, cin, cout, H, W, (relu, bias))
F23_WALK = [(2, 16, 32, 421, 403, (True, True)), (2, 24, 32, 421, 403, (False, False)), (2, 16, 96, 200, 277, (False, True))]


@pytest.mark.parametrize("B,cin,cout,H,W,variant", F23_WALK)
def test_f23_persistent_walk_vs_float64(dev, B, cin, cout, H, W, variant):
    nblk, tall, nw = f23_blocks(B, H, W, cout)
    assert nw == 1 and nblk >= 2.5 * _cus(), (nblk, _cus())
    assert H % 64 and W % 16 and H % 32 and W % 8
    _f23_case(B, cin, cout, H, W, (variant,), what="f23 walk")


def _grouped_inputs(B, H, W, gcin, couts, trailing, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = len(couts)
    x = torch.randn(B, n * gcin + trailing, H, W, generator=g)
    x[:, :, 0, :] += 2.0
    x[:, :, :, -1] -= 3.0
    ws = [torch.randn(c, gcin, 3, 3, generator=g) / math.sqrt(9 * gcin) for c in couts]
    bs = [torch.randn(c, generator=g) for c in couts]
    w_all, b_all = torch.zeros(32 * n, gcin, 3, 3), torch.zeros(32 * n)
    for k, (w, b) in enumerate(zip(ws, bs)):
        w_all[32 * k:32 * k + w.shape[0]], b_all[32 * k:32 * k + w.shape[0]] = w, b
    return x, ws, bs, w_all, b_all


# (B, H, W, group_cin, couts, trailing input channels, persistent walk)
F23_GROUPED = [
    (2, 18, 26, 16, [1, 32, 7, 12, 2], 8, False),
    (1, 9, 35, 24, [32, 1, 5, 31, 8, 3], 4, False),
    (2, 11, 13, 64, [4, 1, 32, 10, 6], 12, False),
    (3, 150, 130, 16, [3, 32, 1, 17, 8, 30], 8, True),
]


@pytest.mark.parametrize("B,H,W,gcin,couts,trailing,walk", F23_GROUPED)
def test_f23_grouped_and_compact_vs_float64(dev, B, H, W, gcin, couts, trailing, walk):
    """group g reads its own slice of a wider input; the padded form writes [32 g, 32 g + 32) into a slice of a wider map, the
    compact form (raw entry point: out_C above the sum of the couts, out_off > 0, no alignment) only the real channels"""
    n, ctot = len(couts), sum(couts)
    if walk:
        assert f23_blocks(B, H, W, 32 * n, grouped=True)[0] >= 2.5 * _cus()
    x, ws, bs, w_all, b_all = _grouped_inputs(B, H, W, gcin, couts, trailing, 31 * gcin + n + H)
    xd, packed, bd = x.to(DEV).contiguous(memory_format=CL), wino.pack_weights(w_all.to(DEV)), b_all.to(DEV)
    relu = not walk
    wants = []
    for k, (w, b) in enumerate(zip(ws, bs)):
        y = _conv_ref(x[:, k * gcin:(k + 1) * gcin], w, b)
        wants.append(torch.relu(y) if relu else y)
    off = 4
    out = _sentinel_map(B, 32 * n + 12, H, W)
    wino.conv3x3_grouped(xd, packed, gcin, n, bd, relu, out=out, out_offset=off)
    for k, c in enumerate(couts):
        _check(out[:, off + 32 * k:off + 32 * k + c], wants[k], f"f23 grouped {(B, H, W, gcin)} group {k}")
        assert not out[:, off + 32 * k + c:off + 32 * (k + 1)].any()                  # padded output channels: zero filters, zero bias
    assert _outside_untouched(out, off, 32 * n)
    # compact, raw: group k at channels [coff + ooff[k], + couts[k]) with a gap of two unowned channels after every group
    coff, out_c = 3, ctot + 2 * n + 7
    ooff = [sum(couts[:k]) + 2 * k for k in range(n)]
    tc, to = torch.tensor(couts, dtype=torch.int32, device=DEV), torch.tensor(ooff, dtype=torch.int32, device=DEV)
    cout_map = _sentinel_map(B, out_c, H, W)
    _lib.check(_lib.lib().lidar_wino_conv3x3_grouped_compact_nhwc(_lib.ptr(xd), B, H, W, xd.shape[1], gcin, n, _lib.ptr(packed), _lib.ptr(bd), int(relu),
                                                                  _lib.ptr(tc), _lib.ptr(to), _lib.ptr(cout_map), out_c, coff, _lib.stream()),
               "lidar_wino_conv3x3_grouped_compact_nhwc")
    owned = torch.zeros(out_c, dtype=torch.bool)
    for k, c in enumerate(couts):
        _check(cout_map[:, coff + ooff[k]:coff + ooff[k] + c], wants[k], f"f23 compact {(B, H, W, gcin)} group {k}")
        assert torch.equal(cout_map[:, coff + ooff[k]:coff + ooff[k] + c], out[:, off + 32 * k:off + 32 * k + c])
        owned[coff + ooff[k]:coff + ooff[k] + c] = True
    assert int((~owned).sum()) == out_c - ctot and bool((cout_map[:, (~owned).to(DEV)] == SENTINEL).all())
    # the Python wrapper (out_C = sum of the couts, no gaps) gives the same channels
    got, _ = wino.conv3x3_grouped_compact(xd, packed, gcin, couts, bd, relu)
    o = 0
    for k, c in enumerate(couts):
        assert torch.equal(got[:, o:o + c], out[:, off + 32 * k:off + 32 * k + c])
        o += c


# ------------------------------------------------------------------ (c) F(4x4, 3x3) (csrc/wino43_conv.hip)
def f43_blocks(B, H, W, cout):
    """-> (n_blocks, tile-group shape) as lidar_wino43_conv3x3_nhwc decides them      csrc/wino43_conv.hip:567-578:
    tiles of 4 x 4 pixels; for (ty, tx) in (4, 4), (2, 8), (8, 2): n = divup(tiles_y, 2 ty) * divup(tiles_x, tx), the first smallest
    wins; n_blocks = B * n * (Cout / 64)"""
    ty, tx = (H + 3) // 4, (W + 3) // 4
    ns = [(_divup(ty, 2 * a) * _divup(tx, b), i) for i, (a, b) in enumerate(((4, 4), (2, 8), (8, 2)))]
    n, best = min(ns)
    return B * n * (cout // 64), ("4x4", "2x8", "8x2")[best]


# Cin in {32, 80, 112} x Cout in {192, 320} (3 and 5 channel groups); (B, cin, cout, H, W, tile-group shape, persistent walk)
F43_CASES = [
    (1, 32, 192, 16, 16, "4x4", False), (2, 80, 320, 6, 40, "2x8", False), (1, 112, 192, 61, 7, "8x2", False),
    (1, 112, 320, 9, 11, "4x4", False), (2, 80, 192, 1, 1, "4x4", False), (1, 32, 320, 35, 66, "2x8", False),
    (2, 32, 192, 215, 250, "4x4", True),
]


@pytest.mark.parametrize("B,cin,cout,H,W,shape,walk", F43_CASES)
def test_f43_sweep_vs_float64(dev, B, cin, cout, H, W, shape, walk):
    """reads channels [0, cin) of a wider input, writes an offset slice of a wider map"""
    nblk, got_shape = f43_blocks(B, H, W, cout)
    assert got_shape == shape
    if walk:
        assert nblk >= 2.5 * _cus(), (nblk, _cus())
    x, w, bias = _conv_inputs(B, cin + 8, cin, cout, H, W, 1000 * cin + cout + 7 * H + W)
    xd, packed, bd = x.to(DEV).contiguous(memory_format=CL), wino.pack_weights43(w.to(DEV)), bias.to(DEV)
    pre = _conv_ref(x[:, :cin], w, bias)
    off = 12
    for relu, wb in (((False, True),) if walk else ALL3):
        p = pre if wb else pre - bias.double().view(1, -1, 1, 1)
        out = _sentinel_map(B, cout + 20, H, W)
        wino.conv3x3_f43(xd, packed, cout, bd if wb else None, relu, out=out, out_offset=off, cin=cin)
        _check(out[:, off:off + cout], torch.relu(p) if relu else p, f"f43 {(B, cin, cout, H, W, relu, wb)}")
        assert _outside_untouched(out, off, cout)


# ------------------------------------------------------------------ (d) the 32-bit limits, on real maps
def _device_map(B, C_, H, W, seed):
    """a channels-last (B, C_, H, W) map drawn on the device from a seeded generator, every frame different"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((B, H, W, C_), generator=g, device=DEV)
    x[:, 0] += 2.0
    x[:, :, -1] -= 3.0
    return x.permute(0, 3, 1, 2)


def _crop_checks(run_name, xd, cin, w, bias, relu, out, off, rows=3):
    """float64 on the CPU: the first frame's top rows and the last frame's bottom rows (each crop with its one-row halo) — where a
    wrapped byte offset would land"""
    B, _, H, W = xd.shape
    cout = w.shape[0]
    for b, r0, r1 in ((0, 0, rows), (B - 1, H - rows, H)):
        h0, h1 = max(r0 - 1, 0), min(r1 + 1, H)
        want = _conv_ref(xd[b:b + 1, :cin, h0:h1].cpu(), w, bias)[:, :, r0 - h0:r0 - h0 + rows]
        _check(out[b:b + 1, off:off + cout, r0:r1], torch.relu(want) if relu else want, f"{run_name} crop frame {b} rows {r0}..{r1}")


def _frames_agree(run_name, big, small_of_frame, B):
    """every frame of the big run against the same entry point run on that frame alone (a view that starts at its own base address):
    the same tiles and the same arithmetic per pixel at other offsets, so the frames must be bit-equal (measured so on an MI355X)"""
    for b in range(B):
        small = small_of_frame(b)
        scale = max(1.0, float(small.abs().max()))
        err = float((big[b:b + 1] - small).abs().max())
        print(f"{run_name}: frame {b} alone: max diff {err:.2e} scale {scale:.1f}")
        assert err <= BAR * scale, (run_name, b, err, scale)
        assert torch.equal(big[b:b + 1], small), (run_name, b, err)
        del small


@pytest.mark.parametrize("side,lim", [("out", F43_OUT_LIMIT), ("in", F43_IN_LIMIT)])
def test_f43_on_maps_within_one_row_of_the_byte_limit(dev, side, lim):
    B, H, W, cin, in_c, cout, out_c = (lim[k] for k in ("B", "H", "W", "cin", "in_c", "cout", "out_c"))
    big_c = out_c if side == "out" else in_c
    assert 2 ** 31 - 1 - W * big_c * 4 < B * H * W * big_c * 4 < 2 ** 31 - 1
    g = torch.Generator(device="cpu").manual_seed(43)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g)
    packed, bd = wino.pack_weights43(w.to(DEV)), bias.to(DEV)
    xd = _device_map(B, in_c, H, W, 4300)
    out = wino.conv3x3_f43(xd, packed, cout, bd, True, cin=cin)
    _crop_checks(f"f43 {side}-limit", xd, cin, w, bias, True, out, 0)
    _frames_agree(f"f43 {side}-limit", out, lambda b: wino.conv3x3_f43(xd[b:b + 1], packed, cout, bd, True, cin=cin), B)
    del out, xd


def test_deconv_on_a_map_within_one_pixel_of_the_byte_limit(dev):
    d = DECONV_LIMIT
    B, K, h, w, s, c_up, out_c = (d[k] for k in ("B", "K", "h", "w", "s", "c_up", "out_c"))
    assert 2 ** 31 - 1 - s * s * out_c * 4 < B * h * w * s * s * out_c * 4 < 2 ** 31 - 1
    g = torch.Generator(device="cpu").manual_seed(44)
    wt = torch.randn(K, c_up, s, s, generator=g) / math.sqrt(K)
    bias = torch.randn(c_up, generator=g)
    w_kn = wt.permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(DEV)
    packed, bd = bb.deconv_pack(w_kn), bias.to(DEV)
    xd = _device_map(B, K, h, w, 4400)
    out = torch.empty((B, out_c, s * h, s * w), device=DEV).contiguous(memory_format=CL)
    bb.deconv_gemm_into_(xd, packed, bd, s, out, 0, True)
    for r0, r1 in ((0, 2), (h - 2, h)):                              # kernel == stride: the crop needs no halo
        want = torch.relu(F.conv_transpose2d(xd[:, :, r0:r1].cpu().double(), wt.double(), bias.double(), stride=s))
        _check(out[:, :, s * r0:s * r1], want, f"deconv limit rows {r0}..{r1}")
    # the whole map: the two-step path (library GEMM + the pixel-shuffle pass with its 64-bit indices)
    ref = torch.empty_like(out)
    y = bb.rows_gemm(xd.permute(0, 2, 3, 1).reshape(B * h * w, K), w_kn)
    bb.bias_act_upsample_(y, bd, B, h, w, s, ref, 0, True)
    del y
    scale = max(1.0, float(ref.abs().max()))
    err = float((out - ref).abs().max())
    print(f"deconv limit vs two-step path: max err {err:.2e} scale {scale:.1f}, bit-equal: {torch.equal(out, ref)}")
    assert err <= BAR * scale
    # ... and the kernel's own small-map behaviour, row band by row band (kernel == stride: bands are independent)
    bands = [(r, min(r + 128, h)) for r in range(0, h, 128)]

    def band(i):
        r0, r1 = bands[i]
        xb = xd[:, :, r0:r1].contiguous(memory_format=CL)
        ob = torch.empty((B, out_c, s * (r1 - r0), s * w), device=DEV).contiguous(memory_format=CL)
        return bb.deconv_gemm_into_(xb, packed, bd, s, ob, 0, True)
    for i, (r0, r1) in enumerate(bands):                            # a pixel's sums do not depend on where it lies: bit-equal
        small = band(i)
        part = out[:, :, s * r0:s * r1]
        err = float((part - small).abs().max())
        print(f"deconv limit: rows {r0}..{r1} alone: max diff {err:.2e}")
        assert err <= BAR * scale, (i, err)
        assert torch.equal(part, small), (i, err)
    del out, ref, xd


@pytest.mark.parametrize("route,B,cin,cout,H,W", [("auto", 9, 32, 64, 1024, 1024), ("direct", 9, 16, 32, 1024, 2048)])
def test_f23_on_a_map_over_two_gib(dev, monkeypatch, route, B, cin, cout, H, W):
    """the oversize route of wino.conv3x3_auto on a real output map of more than 2^31 bytes (size_t addressing in the F(2x2) kernel):
    through conv3x3_auto with the filters of pack_auto for the smallest layer F(4x4) takes, and at the smallest (Cin, Cout) directly"""
    assert B * H * W * cout * 4 > 2 ** 31
    g = torch.Generator(device="cpu").manual_seed(45)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g)
    bd = bias.to(DEV)
    xd = _device_map(B, cin, H, W, 4500)
    if route == "auto":
        packed = wino.pack_auto(w.to(DEV))
        assert packed[0] == "f43" and not wino.f43_fits(xd.shape, cout)
        calls = {"f43": 0, "f23": 0}

        def count(name, fn):
            def wrapped(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return wrapped
        f23 = wino.conv3x3
        monkeypatch.setattr(wino, "conv3x3_f43", count("f43", wino.conv3x3_f43))
        monkeypatch.setattr(wino, "conv3x3", count("f23", f23))
        out = wino.conv3x3_auto(xd, packed, cout, bd, True)
        assert calls == {"f43": 0, "f23": 1}, calls
        p23 = packed[3]
    else:
        f23, p23 = wino.conv3x3, wino.pack_weights(w.to(DEV))
        out = f23(xd, p23, cout, bd, True)
    assert out.numel() * 4 > 2 ** 31
    _crop_checks(f"f23 oversize {route}", xd, cin, w, bias, True, out, 0)
    _frames_agree(f"f23 oversize {route}", out, lambda b: f23(xd[b:b + 1], p23, cout, bd, True), B)
    del out, xd


# ------------------------------------------------------------------ (e) the epilogue passes and the library GEMM wrapper
# n4 = pixels * C / 4 float4 per launch, 1024 per workgroup: n4 % 1024 in {1, 255, 257, 1023}; w = 1, h = 1; (shape, out_C, off, relu)
@pytest.mark.parametrize("shape,out_c,off,relu", [
    ((1, 4, 1, 1025), 12, 4, True), ((1, 4, 255, 1), 8, 4, False), ((1, 4, 1, 257), 4, 0, True), ((3, 4, 341, 1), 16, 8, False),
    ((1, 12, 683, 1), 20, 4, True), ((1, 20, 1, 51), 28, 8, False), ((1, 8, 1, 1), 16, 8, True),
])
def test_bias_act_tails_bit_exact(dev, shape, out_c, off, relu):
    B, C_, H, W = shape
    n4 = B * H * W * C_ // 4
    assert n4 % 1024 in (1, 255, 257, 1023) or n4 < 1024
    g = torch.Generator(device="cpu").manual_seed(7 + C_ + W)
    x = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=CL)
    b = torch.randn(C_, generator=g).to(DEV)
    want = x + b.view(1, -1, 1, 1)
    want = torch.relu(want) if relu else want
    out = _sentinel_map(B, out_c, H, W)
    bb.bias_act_(x, b, relu=relu, out=out, out_offset=off)
    assert torch.equal(out[:, off:off + C_], want) and _outside_untouched(out, off, C_)
    assert torch.equal(bb.bias_act_(x.clone(memory_format=CL), b, relu=relu), want)            # in place


# n4 = B h w s s C / 4; (B, h, w, s, C, out_C, off, relu)
@pytest.mark.parametrize("B,h,w,s,C_,out_c,off,relu", [
    (1, 569, 1, 3, 4, 12, 4, True), (1, 1, 711, 3, 4, 8, 4, False), (3, 275, 1, 3, 4, 4, 0, True), (5, 7, 13, 3, 4, 16, 8, False),
    (1, 1, 1025, 1, 4, 8, 4, True), (1, 255, 1, 1, 4, 12, 8, False), (1, 1, 257, 1, 4, 8, 0, True), (3, 11, 31, 1, 4, 8, 4, False),
    (2, 3, 5, 3, 8, 24, 12, True), (1, 1, 1, 3, 12, 16, 4, False),
])
def test_bias_act_upsample_tails_bit_exact(dev, B, h, w, s, C_, out_c, off, relu):
    n4 = B * h * w * s * s * C_ // 4
    assert n4 % 1024 in (1, 255, 257, 1023) or n4 < 1024
    g = torch.Generator(device="cpu").manual_seed(11 + h + w + s)
    y = torch.randn(B * h * w, s * s * C_, generator=g).to(DEV)
    b = torch.randn(C_, generator=g).to(DEV)
    want = y.view(B, h, w, s, s, C_) + b
    want = (torch.relu(want) if relu else want).permute(0, 5, 1, 3, 2, 4).reshape(B, C_, h * s, w * s)
    out = _sentinel_map(B, out_c, h * s, w * s)
    bb.bias_act_upsample_(y, b, B, h, w, s, out, off, relu)
    assert torch.equal(out[:, off:off + C_], want) and _outside_untouched(out, off, C_)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,h,w,K,N,out_c,off", [
    (1, 1, 1, 16, 8, 16, 4),             # M = 1
    (1, 127, 1, 64, 72, 80, 8),          # M = 127
    (3, 7, 5, 24, 128, 384, 128),
    (2, 20, 13, 256, 8, 8, 0),           # the slice is the whole map
    (1, 9, 33, 16, 72, 76, 4),
])
def test_gemm_bias_act_into_vs_float64(dev, B, h, w, K, N, out_c, off, relu):
    g = torch.Generator(device="cpu").manual_seed(K + N + h)
    x = torch.randn(B, K, h, w, generator=g)
    wkn = torch.randn(K, N, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    want = x.permute(0, 2, 3, 1).reshape(-1, K).double() @ wkn.double() + bias.double()
    want = torch.relu(want) if relu else want
    out = _sentinel_map(B, out_c, h, w)
    ok = bb.gemm_bias_act_into_(x.to(DEV).contiguous(memory_format=CL), wkn.to(DEV), bias.to(DEV), out, off, relu)
    assert ok is True                                                # the library path is available on these machines
    rows = out.permute(0, 2, 3, 1).reshape(-1, out_c)
    _check(rows[:, off:off + N], want, f"gemm {(B * h * w, K, N, out_c, off, relu)}")
    assert _outside_untouched(out, off, N)
