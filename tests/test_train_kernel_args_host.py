"""CPU checks of the argument rejection of the train-path entry points (csrc/bn_train.hip, csrc/pfn_train.hip,
csrc/wino43_wgrad.hip): the edges of the ranges include/lidar_hip.h declares, from the outside.  Every call below hands the library
fake (never dereferenced) addresses and is refused with LIDAR_ERR_ARG (-1), or LIDAR_ERR_WORKSPACE (-3) for a workspace one byte
short, before anything is launched; tests/test_gpu_train_kernel_support.py runs the inside of the same ranges on the GPU."""
import ctypes as C

from lidardetection_amd import _lib

ERR_ARG, ERR_WORKSPACE = -1, -3
A = 0x20000                                                          # a 16-byte aligned fake address


def _bn(L, backward, nseg=1, ptr=0x10000, dptr=0x30000, ld=64, off=0, c=64, rows=100, m_ld=64, m_off=0, ws=A, ws_bytes=1 << 30):
    """lidar_bn_relu_train_forward / _backward with one description for every segment; m_ld / m_off: y (forward) or grad_y"""
    n = max(nseg, 1)
    xs, dxs = (C.c_void_p * n)(*([ptr] * n)), (C.c_void_p * n)(*([dptr] * n))
    lds, offs, cs = _lib.host_i32([ld] * n), _lib.host_i32([off] * n), _lib.host_i32([c] * n)
    a, w = C.c_void_p(A), C.c_void_p(ws)
    if backward:
        return L.lidar_bn_relu_train_backward(nseg, xs, lds, offs, cs, rows, a, m_ld, m_off, a, a, a, dxs, a, a, w, ws_bytes, None)
    return L.lidar_bn_relu_train_forward(nseg, xs, lds, offs, cs, rows, a, a, 1e-3, a, m_ld, m_off, a, a, a, w, ws_bytes, None)


def test_bn_relu_train_refuses_the_outside_of_its_declared_range():
    L = _lib.lib()
    for backward in (False, True):
        bn = lambda **kw: _bn(L, backward, **kw)                     # noqa: E731
        assert bn(nseg=0) == ERR_ARG and bn(nseg=5) == ERR_ARG       # 1..4 segments
        assert bn(c=2, ld=64) == ERR_ARG                             # below 4 channels
        assert bn(c=1028, ld=1028, m_ld=1028) == ERR_ARG             # above 1024
        assert bn(c=6, ld=64) == ERR_ARG and bn(c=1022, ld=1024, m_ld=1024) == ERR_ARG      # not a multiple of 4
        assert bn(c=64, off=4, ld=64) == ERR_ARG                     # off + C > ld
        assert bn(c=32, off=2, ld=64) == ERR_ARG and bn(c=32, off=-4, ld=64) == ERR_ARG     # off % 4, off < 0
        assert bn(c=32, m_off=2, m_ld=64) == ERR_ARG and bn(c=64, m_off=4, m_ld=64) == ERR_ARG
        assert bn(ptr=0x10004) == ERR_ARG                            # a map misaligned by 4 bytes
        assert bn(ws=A + 4) == ERR_ARG
        assert bn(rows=1) == ERR_ARG and bn(rows=0) == ERR_ARG       # one value per channel: torch refuses it too
        need = L.lidar_bn_relu_train_workspace_bytes(100, 64)
        assert need > 0 and bn(ws_bytes=need - 1) == ERR_WORKSPACE
        n4 = L.lidar_bn_relu_train_workspace_bytes(100, 4 * 64)      # the workspace is sized by the concatenated width
        assert bn(nseg=4, m_ld=256, ws_bytes=n4 - 1) == ERR_WORKSPACE
    assert _bn(L, True, dptr=0x30004) == ERR_ARG                     # a misaligned dz buffer


def _pfn(L, backward, V=10, P=32, nf=4, cout=64, dist=0, ws_bytes=1 << 30):
    a = C.c_void_p(A)
    vs, rg = _lib.host_f32([0.16, 0.16, 4.0]), _lib.host_f32([0, -39.68, -3, 69.12, 39.68, 1])
    if backward:
        return L.lidar_pfn_train_backward(a, a, a, V, None, P, nf, a, a, cout, vs, rg, dist, 0, 0, a, a, a, a, a, a, a, a, a, ws_bytes, None)
    return L.lidar_pfn_train_forward(a, a, a, V, None, P, nf, a, a, a, cout, 1e-3, vs, rg, dist, 0, 0, a, a, a, a, a, a, a, ws_bytes, None)


def test_pfn_train_refuses_the_outside_of_its_declared_range():
    L = _lib.lib()
    for backward in (False, True):
        pfn = lambda **kw: _pfn(L, backward, **kw)                   # noqa: E731
        assert pfn(nf=2) == ERR_ARG and pfn(nf=9) == ERR_ARG         # 3..8 point features
        assert pfn(P=0) == ERR_ARG and pfn(P=65) == ERR_ARG          # 1..64 points: one wave
        assert pfn(cout=0) == ERR_ARG and pfn(cout=65) == ERR_ARG    # 1..64 channels: one wave
        assert pfn(V=0) == ERR_ARG
        for nf, dist in ((3, 0), (8, 1)):
            need = L.lidar_pfn_train_workspace_bytes(10, nf, 64, dist)
            assert need > 0 and pfn(nf=nf, dist=dist, ws_bytes=need - 1) == ERR_WORKSPACE


def test_scatter_backward_and_wgrad_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    a = C.c_void_p(A)
    for ch in (16, 48, 96, 256):
        assert L.lidar_pillar_scatter_backward(a, a, 0, 10, None, ch, 1, 8, 8, 0, a, None) == ERR_ARG
    assert L.lidar_pillar_scatter_backward(a, a, 0, 10, None, 64, 0, 8, 8, 0, a, None) == ERR_ARG
    assert L.lidar_pillar_scatter_backward(a, a, 0, 10, None, 64, 1, 0, 8, 0, a, None) == ERR_ARG
    wg = lambda cin, cout, x_ld, g_ld, H=8, W=8: L.lidar_wino43_wgrad_nhwc(a, x_ld, a, g_ld, 2, H, W, cin, cout, a, a, 1 << 40, None)   # noqa: E731
    assert wg(16, 64, 16, 64) == ERR_ARG and wg(64, 544, 64, 544) == ERR_ARG and wg(48, 64, 48, 64) == ERR_ARG
    assert wg(64, 128, 60, 128) == ERR_ARG and wg(64, 128, 64, 124) == ERR_ARG      # a row stride below the channel count
    assert wg(64, 64, 64, 64, H=0) == ERR_ARG and wg(64, 64, 64, 64, W=0) == ERR_ARG
    need = L.lidar_wino43_wgrad_workspace_bytes(2, 8, 8, 32, 512)
    assert need > 0 and L.lidar_wino43_wgrad_nhwc(a, 40, a, 520, 2, 8, 8, 32, 512, a, a, need - 1, None) == ERR_WORKSPACE
    assert L.lidar_wino43_wgrad_supported(32, 512) and L.lidar_wino43_wgrad_supported(512, 32) and L.lidar_wino43_wgrad_supported(96, 160)
