"""CPU checks of the argument rejection of the dense inference BEV entry points (csrc/wino_conv.hip, csrc/wino43_conv.hip,
csrc/deconv_gemm.hip, csrc/dense_epilogue.hip, csrc/dense_gemm.hip): the edges of the ranges include/lidar_hip.h declares, from the
outside.  Every launch call below hands the library fake (never dereferenced) addresses and is refused with LIDAR_ERR_ARG (-1) before
anything is launched; tests/test_gpu_bev_kernel_support.py runs the inside of the same ranges on the GPU."""
import ctypes as C

from lidardetection_amd import _lib
from lidardetection_amd import bev_backbone as bb
from lidardetection_amd import wino

ERR_ARG = -1
A = 0x20000                                                          # a 16-byte aligned fake address

# the largest maps tests/test_gpu_bev_kernel_support.py runs (its section (d)).  BOTH files depend on these dicts: the GPU file imports
# them and runs exactly these shapes, this file checks that they are accepted and that one pixel (row) more is refused, so the
# accepted / refused pair is stated once.  Change them only together with both files.
DECONV_LIMIT = dict(K=16, s=4, c_up=128, out_c=128, B=1, h=511, w=513)          # P = 262 143: 2^31 - 8192 output bytes
F43_OUT_LIMIT = dict(cin=32, in_c=32, cout=64, out_c=64, B=7, H=889, W=1348)     # B H W = 8 388 604 (8 388 607 is the last one accepted)
F43_IN_LIMIT = dict(cin=32, in_c=128, cout=64, out_c=64, B=3, H=1025, W=1364)    # B H W = 4 194 300 (4 194 303 is the last one accepted)


def _a(v=A):
    return C.c_void_p(v)


def test_supported_predicates_and_packed_sizes_at_their_edges():
    L = _lib.lib()
    # F(2x2): Cin % 8 == 0, Cin >= 16, Cout % 32 == 0
    for cin, cout in ((8, 32), (12, 32), (20, 32), (16, 48), (16, 0), (0, 32), (-16, 32), (16, -32), (16, 16)):
        assert not L.lidar_wino_supported(cin, cout) and L.lidar_wino_packed_floats(cin, cout) == 0, (cin, cout)
    for cin, cout in ((16, 32), (24, 32), (40, 96), (64, 160), (16, 192), (512, 1152)):
        assert L.lidar_wino_supported(cin, cout) and L.lidar_wino_packed_floats(cin, cout) == 16 * cin * cout, (cin, cout)
    # F(4x4): Cin % 16 == 0, Cin >= 32, Cout % 64 == 0
    for cin, cout in ((16, 64), (40, 64), (24, 64), (32, 32), (32, 96), (32, 0), (0, 64), (-32, 64), (32, -64)):
        assert not L.lidar_wino43_supported(cin, cout) and L.lidar_wino43_packed_floats(cin, cout) == 0, (cin, cout)
        assert not wino.supported43(cin, cout)
    for cin, cout in ((32, 64), (48, 64), (80, 192), (112, 320), (256, 256)):
        assert L.lidar_wino43_supported(cin, cout) and L.lidar_wino43_packed_floats(cin, cout) == 36 * cin * cout, (cin, cout)
    # deblock: K % 8 == 0, K >= 16, C_up % 128 == 0, (s s C_up) % 512 == 0
    for K, s, c_up in ((8, 2, 128), (20, 2, 128), (12, 2, 128), (16, 2, 64), (16, 2, 192), (16, 3, 128), (16, 1, 128), (16, 1, 384),
                       (16, 0, 512), (16, -2, 128), (16, 2, 0), (0, 2, 128), (-16, 2, 128)):
        assert not L.lidar_deconv_supported(K, s, c_up), (K, s, c_up)
        assert not bb.deconv_supported(K, s, c_up)
    for K, N in ((8, 512), (20, 512), (16, 256), (16, 768), (16, 1152), (16, 0), (0, 512)):      # 1152 = 3 * 3 * 128
        assert L.lidar_deconv_packed_floats(K, N) == 0, (K, N)
    for K, s, c_up in ((16, 8, 128), (24, 2, 384), (40, 1, 512), (64, 3, 512), (256, 4, 256), (16, 2, 128)):
        assert L.lidar_deconv_supported(K, s, c_up) and L.lidar_deconv_packed_floats(K, s * s * c_up) == K * s * s * c_up, (K, s, c_up)


def _f23(L, B=2, H=8, W=8, cin=16, cout=32, out_c=32, off=0, inp=A, packed=A, out=A):
    return L.lidar_wino_conv3x3_nhwc(_a(inp), B, H, W, cin, _a(packed), None, 0, cout, _a(out), out_c, off, None)


def _f23g(L, compact, B=2, H=8, W=8, in_c=96, gcin=16, n=5, out_c=None, off=0, inp=A, packed=A, out=A, tables=(A, A)):
    if compact:
        return L.lidar_wino_conv3x3_grouped_compact_nhwc(_a(inp), B, H, W, in_c, gcin, n, _a(packed), None, 0, _a(tables[0]), _a(tables[1]),
                                                         _a(out), 40 if out_c is None else out_c, off, None)
    return L.lidar_wino_conv3x3_grouped_nhwc(_a(inp), B, H, W, in_c, gcin, n, _a(packed), None, 0, _a(out), 32 * max(n, 0) if out_c is None else out_c,
                                             off, None)


def test_f23_launchers_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    f = lambda **kw: _f23(L, **kw)                                   # noqa: E731
    assert f(B=0) == ERR_ARG and f(H=0) == ERR_ARG and f(W=0) == ERR_ARG and f(B=-1) == ERR_ARG and f(H=-3) == ERR_ARG and f(W=-3) == ERR_ARG
    for cin in (8, 12, 20):
        assert f(cin=cin) == ERR_ARG
    assert f(cout=48, out_c=48) == ERR_ARG and f(cout=0, out_c=32) == ERR_ARG
    assert f(out_c=64, off=36) == ERR_ARG                            # off + Cout > out_C
    assert f(out_c=64, off=2) == ERR_ARG and f(out_c=64, off=-4) == ERR_ARG
    assert f(out_c=34) == ERR_ARG and f(out_c=38, off=4) == ERR_ARG  # out_C % 4
    assert f(inp=A + 4) == ERR_ARG and f(packed=A + 4) == ERR_ARG and f(out=A + 4) == ERR_ARG and f(out=A + 8) == ERR_ARG
    assert f(inp=0) == ERR_ARG and f(packed=0) == ERR_ARG and f(out=0) == ERR_ARG
    for compact in (False, True):
        g = lambda **kw: _f23g(L, compact, **kw)                     # noqa: E731
        assert g(in_c=76) == ERR_ARG                                 # group_cin * n_groups > in_C
        assert g(n=7) == ERR_ARG and g(n=0) == ERR_ARG and g(n=-1) == ERR_ARG
        assert g(gcin=8, in_c=96) == ERR_ARG and g(gcin=20, in_c=128) == ERR_ARG and g(gcin=0) == ERR_ARG
        assert g(in_c=94) == ERR_ARG and g(in_c=82) == ERR_ARG       # in_C % 4
        assert g(B=0) == ERR_ARG and g(H=0) == ERR_ARG and g(W=0) == ERR_ARG
        assert g(off=-4) == ERR_ARG and g(off=-1) == ERR_ARG
        assert g(inp=A + 4) == ERR_ARG and g(packed=A + 4) == ERR_ARG and g(inp=0) == ERR_ARG and g(packed=0) == ERR_ARG and g(out=0) == ERR_ARG
    g = lambda **kw: _f23g(L, False, **kw)                           # noqa: E731
    assert g(out_c=164, off=8) == ERR_ARG and g(out_c=164, off=2) == ERR_ARG and g(out_c=162) == ERR_ARG and g(out=A + 4) == ERR_ARG
    g = lambda **kw: _f23g(L, True, **kw)                            # noqa: E731
    assert g(tables=(0, A)) == ERR_ARG and g(tables=(A, 0)) == ERR_ARG and g(tables=(0, 0)) == ERR_ARG


def _f43(L, B=2, H=8, W=8, cin=32, in_c=32, cout=64, out_c=64, off=0, inp=A, packed=A, out=A):
    return L.lidar_wino43_conv3x3_nhwc(_a(inp), B, H, W, cin, in_c, _a(packed), None, 0, cout, _a(out), out_c, off, None)


def test_f43_launcher_refuses_the_outside_of_its_declared_range_and_the_first_map_too_large():
    L = _lib.lib()
    f = lambda **kw: _f43(L, **kw)                                   # noqa: E731
    assert f(B=0) == ERR_ARG and f(H=0) == ERR_ARG and f(W=0) == ERR_ARG and f(B=-1) == ERR_ARG and f(H=-3) == ERR_ARG and f(W=-3) == ERR_ARG
    assert f(cin=16, in_c=16) == ERR_ARG and f(cin=40, in_c=40) == ERR_ARG and f(cin=24, in_c=32) == ERR_ARG
    assert f(cout=32, out_c=64) == ERR_ARG and f(cout=96, out_c=96) == ERR_ARG
    assert f(out_c=96, off=36) == ERR_ARG and f(out_c=96, off=2) == ERR_ARG and f(out_c=96, off=-4) == ERR_ARG
    assert f(out_c=66) == ERR_ARG and f(out_c=70, off=4) == ERR_ARG  # out_C % 4
    assert f(in_c=34) == ERR_ARG and f(in_c=38) == ERR_ARG           # in_C % 4
    assert f(in_c=28) == ERR_ARG and f(cin=64, in_c=32) == ERR_ARG   # in_C < Cin
    assert f(inp=A + 4) == ERR_ARG and f(packed=A + 4) == ERR_ARG and f(out=A + 4) == ERR_ARG and f(out=A + 8) == ERR_ARG
    assert f(inp=0) == ERR_ARG and f(packed=0) == ERR_ARG and f(out=0) == ERR_ARG
    # the byte limits: what the GPU file runs fits by wino.f43_fits' arithmetic (an `out` of out_c channels), the last pixel count
    # that fits is 2^31 / (4 C) - 1, and one pixel more is refused — output side (64 channels), then input side (128 channels)
    for lim, c, side in ((F43_OUT_LIMIT, 64, "out"), (F43_IN_LIMIT, 128, "in")):
        last = 2 ** 31 // (4 * c) - 1
        npix = lim["B"] * lim["H"] * lim["W"]
        assert last - lim["W"] < npix <= last                       # the GPU case lies within one row of the limit
        fits = lambda b, h, w: (b * lim["in_c"] * h * w * 4 < wino._F43_MAX_BYTES[0]         # noqa: E731
                                and b * lim["out_c"] * h * w * 4 < wino._F43_MAX_BYTES[0])
        assert wino._F43_MAX_BYTES[0] == 2 ** 31 - 1 and fits(lim["B"], lim["H"], lim["W"]) and fits(1, 1, last) and not fits(1, 1, last + 1)
        assert wino.f43_fits((1, lim["in_c"], 1, last), lim["out_c"]) and not wino.f43_fits((1, lim["in_c"], 1, last + 1), lim["out_c"])
        kw = dict(cin=lim["cin"], in_c=lim["in_c"], cout=lim["cout"], out_c=lim["out_c"])
        assert f(B=1, H=1, W=last + 1, **kw) == ERR_ARG, side
        assert f(B=1, H=last + 1, W=1, **kw) == ERR_ARG and f(B=last + 1, H=1, W=1, **kw) == ERR_ARG, side
        assert f(B=lim["B"], H=lim["H"] + 1, W=lim["W"], **kw) == ERR_ARG, side       # one row more than the GPU case
    assert f(B=1, H=1, W=2 ** 31 // 256 - 1, out_c=68) == ERR_ARG    # fits as a 64-channel map, not as the 68-channel map it is written into


def _dc(L, B=2, h=4, w=4, K=16, s=2, c_up=128, out_c=128, off=0, inp=A, packed=A, out=A):
    return L.lidar_deconv_gemm_nhwc(_a(inp), B, h, w, K, _a(packed), None, 0, s, c_up, _a(out), out_c, off, None)


def test_deconv_launcher_refuses_the_outside_of_its_declared_range_and_the_first_map_too_large():
    L = _lib.lib()
    f = lambda **kw: _dc(L, **kw)                                    # noqa: E731
    assert f(B=0) == ERR_ARG and f(h=0) == ERR_ARG and f(w=0) == ERR_ARG and f(B=-1) == ERR_ARG and f(h=-2) == ERR_ARG and f(w=-2) == ERR_ARG
    assert f(K=8) == ERR_ARG and f(K=20) == ERR_ARG and f(K=0) == ERR_ARG
    assert f(c_up=64, out_c=64) == ERR_ARG and f(c_up=192, out_c=192) == ERR_ARG and f(s=3) == ERR_ARG and f(s=1) == ERR_ARG and f(s=0) == ERR_ARG
    assert f(out_c=256, off=132) == ERR_ARG and f(out_c=256, off=2) == ERR_ARG and f(out_c=256, off=-4) == ERR_ARG
    assert f(out_c=130) == ERR_ARG and f(out_c=134, off=4) == ERR_ARG                 # out_C % 4
    assert f(inp=A + 4) == ERR_ARG and f(packed=A + 4) == ERR_ARG and f(out=A + 4) == ERR_ARG and f(out=A + 8) == ERR_ARG
    assert f(inp=0) == ERR_ARG and f(packed=0) == ERR_ARG and f(out=0) == ERR_ARG
    d = DECONV_LIMIT
    P = d["B"] * d["h"] * d["w"]
    assert P == 2 ** 31 // (4 * d["s"] ** 2 * d["out_c"]) - 1 == 262143
    assert bb._DECONV_MAX_BYTES[0] == 2 ** 31 - 1 and bb.deconv_fits(d["B"], d["K"], d["h"], d["w"], d["s"], d["out_c"])
    assert bb.deconv_fits(1, d["K"], 1, P, d["s"], d["out_c"]) and not bb.deconv_fits(1, d["K"], 1, P + 1, d["s"], d["out_c"])
    kw = dict(K=d["K"], s=d["s"], c_up=d["c_up"], out_c=d["out_c"])
    assert f(B=1, h=1, w=P + 1, **kw) == ERR_ARG and f(B=1, h=P + 1, w=1, **kw) == ERR_ARG and f(B=P + 1, h=1, w=1, **kw) == ERR_ARG
    assert f(B=1, h=512, w=512, **kw) == ERR_ARG
    assert f(B=1, h=1, w=P, K=16, s=4, c_up=128, out_c=132) == ERR_ARG               # fits as a 128-channel map, not as the 132-channel one
    # the input side: K = 1024 at s = 2 into 128 channels — the input map is twice the output map
    Pin = 2 ** 31 // (4 * 1024) - 1
    assert bb.deconv_fits(1, 1024, 1, Pin, 2, 128) and not bb.deconv_fits(1, 1024, 1, Pin + 1, 2, 128)
    assert f(B=1, h=1, w=Pin + 1, K=1024, s=2, c_up=128, out_c=128) == ERR_ARG


def test_epilogue_passes_and_the_library_gemm_refuse_bad_arguments():
    L = _lib.lib()
    a = _a()
    ba = lambda n_pix=10, C=8, out_c=16, off=0: L.lidar_bias_act_nhwc(a, a, n_pix, C, 1, a, out_c, off, None)       # noqa: E731
    assert ba(C=6) == ERR_ARG and ba(C=2) == ERR_ARG and ba(C=0) == ERR_ARG and ba(C=-4) == ERR_ARG
    assert ba(out_c=14) == ERR_ARG and ba(off=2) == ERR_ARG and ba(off=-4) == ERR_ARG
    assert ba(off=12) == ERR_ARG and ba(C=16, out_c=16, off=4) == ERR_ARG and ba(C=8, out_c=4) == ERR_ARG          # slice overflow
    assert ba(n_pix=-1) == ERR_ARG
    assert L.lidar_bias_act_nhwc(None, a, 10, 8, 1, a, 16, 0, None) == ERR_ARG and L.lidar_bias_act_nhwc(a, None, 10, 8, 1, a, 16, 0, None) == ERR_ARG
    assert L.lidar_bias_act_nhwc(a, a, 10, 8, 1, None, 16, 0, None) == ERR_ARG
    up = lambda batch=2, h=3, w=3, s=2, C=8, out_c=16, off=0: L.lidar_bias_act_upsample_nhwc(a, a, batch, h, w, s, C, 1, a, out_c, off, None)   # noqa: E731
    assert up(C=6) == ERR_ARG and up(C=2) == ERR_ARG and up(C=0) == ERR_ARG
    assert up(out_c=14) == ERR_ARG and up(off=2) == ERR_ARG and up(off=-4) == ERR_ARG
    assert up(off=12) == ERR_ARG and up(C=16, out_c=16, off=4) == ERR_ARG and up(C=8, out_c=4) == ERR_ARG          # slice overflow
    assert up(s=0) == ERR_ARG and up(s=-1) == ERR_ARG and up(h=0) == ERR_ARG and up(w=0) == ERR_ARG and up(batch=-1) == ERR_ARG
    assert L.lidar_bias_act_upsample_nhwc(None, a, 2, 3, 3, 2, 8, 1, a, 16, 0, None) == ERR_ARG
    assert L.lidar_bias_act_upsample_nhwc(a, None, 2, 3, 3, 2, 8, 1, a, 16, 0, None) == ERR_ARG
    assert L.lidar_bias_act_upsample_nhwc(a, a, 2, 3, 3, 2, 8, 1, None, 16, 0, None) == ERR_ARG
    gm = lambda M=10, K=16, N=8, ldd=8, relu=0, bias=A, A_=A, W=A, D=A: L.lidar_dense_gemm_bias_act(     # noqa: E731
        _a(A_), M, K, _a(W), N, None if bias is None else _a(bias), relu, _a(D), ldd, None, 0, None)
    assert gm(ldd=7) == ERR_ARG and gm(N=72, ldd=64) == ERR_ARG      # ldd < N
    assert gm(relu=1, bias=None) == ERR_ARG                          # relu without bias
    assert gm(M=0) == ERR_ARG and gm(M=-1) == ERR_ARG and gm(K=0) == ERR_ARG and gm(K=-16) == ERR_ARG and gm(N=0) == ERR_ARG and gm(N=-8) == ERR_ARG
    assert gm(A_=0) == ERR_ARG and gm(W=0) == ERR_ARG and gm(D=0) == ERR_ARG
