"""CPU checks of the SECOND training step's entry points (csrc/sparse_train.hip, the residual form in csrc/bn_train.hip): the edges of
the ranges include/lidar_hip.h declares, from the outside, with fake (never dereferenced) addresses, in the style of
tests/test_train_kernel_args_host.py; and SECONDKitti.train_loss's option checks, which run before anything touches a device.
tests/test_gpu_second_train.py runs the inside of the same ranges on the GPU."""
import ctypes as C

import pytest
import torch

from lidardetection_amd import _lib, spconv

ERR_ARG, ERR_WORKSPACE, OK = -1, -3, 0
A = 0x20000                                                          # a 16-byte aligned fake address


def _gather(L, g=A, idx=A, df=A, g_ld=256, g_off=0, n=10, c=128, B=2, D=2, H=4, W=4):
    p = lambda v: C.c_void_p(v) if v else None                       # noqa: E731
    return L.lidar_sparse_to_bev_nhwc_backward(p(g), g_ld, g_off, p(idx), n, c, B, D, H, W, p(df), None)


def test_bev_gather_backward_refuses_the_outside_of_its_declared_range():
    L = _lib.lib()
    assert _gather(L, g=0) == ERR_ARG and _gather(L, idx=0) == ERR_ARG and _gather(L, df=0) == ERR_ARG      # null pointers
    assert _gather(L, D=0) == ERR_ARG and _gather(L, D=5, g_ld=640) == ERR_ARG                              # 1 <= D <= 4
    assert _gather(L, c=6, g_ld=64) == ERR_ARG and _gather(L, c=0) == ERR_ARG                               # C % 4 == 0
    assert _gather(L, g_ld=255) == ERR_ARG                                                                  # g_ld < C * D
    assert _gather(L, g_ld=256, g_off=4) == ERR_ARG and _gather(L, g_off=-4, g_ld=512) == ERR_ARG            # the slice leaves the row
    assert _gather(L, n=-1) == ERR_ARG and _gather(L, B=0) == ERR_ARG and _gather(L, H=0) == ERR_ARG and _gather(L, W=0) == ERR_ARG
    assert _gather(L, idx=A + 4) == ERR_ARG and _gather(L, df=A + 8) == ERR_ARG and _gather(L, g=A + 2) == ERR_ARG
    # n = 0: success, and nothing is launched (no device is needed for this call to return)
    assert _gather(L, n=0) == OK and _gather(L, n=0, g_ld=300, g_off=44) == OK
    for d in (1, 2, 3, 4):
        assert _gather(L, n=0, D=d, c=4, g_ld=4 * d) == OK


def _bn_add(L, backward, x=A, r=A, dx=A, dr=A, c=64, rows=100, x_ld=64, r_ld=64, m_ld=64, dr_ld=64, ws=A, ws_bytes=1 << 30):
    """lidar_bn_add_relu_train_forward / _backward; m_ld: y (forward) or grad_y (backward)"""
    p = lambda v: C.c_void_p(v) if v else None                       # noqa: E731
    a = C.c_void_p(A)
    if backward:
        return L.lidar_bn_add_relu_train_backward(p(x), x_ld, p(r), r_ld, c, rows, a, m_ld, a, a, a, p(dx), p(dr), dr_ld, a, a, p(ws),
                                                  ws_bytes, None)
    return L.lidar_bn_add_relu_train_forward(p(x), x_ld, p(r), r_ld, c, rows, a, a, 1e-3, a, m_ld, a, a, a, p(ws), ws_bytes, None)


def test_bn_add_relu_train_refuses_the_outside_of_its_declared_range():
    L = _lib.lib()
    for backward in (False, True):
        bn = lambda **kw: _bn_add(L, backward, **kw)                 # noqa: E731
        assert bn(x=0) == ERR_ARG and bn(r=0) == ERR_ARG and bn(ws=0) == ERR_ARG                            # null pointers
        assert bn(rows=1) == ERR_ARG and bn(rows=0) == ERR_ARG       # one value per channel: torch refuses it too
        assert bn(c=6) == ERR_ARG and bn(c=2) == ERR_ARG             # C % 4 == 0, C >= 4
        assert bn(c=1028, x_ld=1028, r_ld=1028, m_ld=1028, dr_ld=1028) == ERR_ARG                           # above 1024
        assert bn(x_ld=60) == ERR_ARG and bn(r_ld=60) == ERR_ARG and bn(m_ld=60) == ERR_ARG                 # a stride below C
        assert bn(x_ld=66) == ERR_ARG and bn(r_ld=66) == ERR_ARG and bn(m_ld=66) == ERR_ARG                 # stride % 4
        assert bn(x=A + 4) == ERR_ARG and bn(r=A + 4) == ERR_ARG and bn(ws=A + 4) == ERR_ARG                # misaligned
        need = L.lidar_bn_relu_train_workspace_bytes(100, 64)
        assert need > 0 and bn(ws_bytes=need - 1) == ERR_WORKSPACE
    bwd = lambda **kw: _bn_add(L, True, **kw)                        # noqa: E731
    assert bwd(dx=0) == ERR_ARG and bwd(dr=0) == ERR_ARG and bwd(dx=A + 4) == ERR_ARG and bwd(dr=A + 4) == ERR_ARG
    assert bwd(dr_ld=60) == ERR_ARG and bwd(dr_ld=66) == ERR_ARG


def test_plain_bn_relu_rows_refuse_one_row():
    """the sparse entry calls lidar_bn_relu_train_* with nseg = 1, rows = N, ld = C: N = 1 is refused there"""
    L = _lib.lib()
    one = lambda v, t=C.c_int: (t * 1)(v)                            # noqa: E731
    a = C.c_void_p(A)
    for c in (16, 32, 64, 128):
        args = (1, one(A, C.c_void_p), one(c), one(0), one(c))
        assert L.lidar_bn_relu_train_forward(*args, 1, a, a, 1e-3, a, c, 0, a, a, a, a, 1 << 30, None) == ERR_ARG
        assert L.lidar_bn_relu_train_backward(*args, 1, a, c, 0, a, a, a, one(A, C.c_void_p), a, a, a, 1 << 30, None) == ERR_ARG


def test_fused_bn_train_is_opt_in_and_restores_its_state():
    assert not spconv.train.fused_bn_train_enabled()
    with spconv.fused_bn_train():
        assert spconv.train.fused_bn_train_enabled()
        with spconv.fused_bn_train(False):
            assert not spconv.train.fused_bn_train_enabled()
        assert spconv.train.fused_bn_train_enabled()
    with pytest.raises(RuntimeError):
        with spconv.fused_bn_train():
            raise RuntimeError("x")
    assert not spconv.train.fused_bn_train_enabled()
    bn = torch.nn.BatchNorm1d(64, eps=1e-3, momentum=0.01)
    assert spconv.train.bn_supported(bn) and not spconv.train.bn_supported(bn.eval())
    bn.train()
    assert not spconv.train.takes(bn, torch.zeros(5, 64))            # CPU features stay on the module
    assert not spconv.train.bn_supported(torch.nn.BatchNorm1d(6)) and not spconv.train.bn_supported(torch.nn.BatchNorm1d(64, momentum=None))
    assert not spconv.train.bn_supported(torch.nn.BatchNorm1d(64, affine=False))
    assert not spconv.train.bn_supported(torch.nn.BatchNorm1d(64, track_running_stats=False))


def test_second_train_loss_refuses_bad_options_before_any_device_work():
    from lidardetection_amd.second import DENSE_HEAD_CFG, SECONDKitti
    model = SECONDKitti(batch_size=2, max_voxels=2000, device="cpu")
    assert SECONDKitti.train_step is __import__("lidardetection_amd.pointpillar", fromlist=["x"]).PointPillarKITTI.train_step
    with pytest.raises(_lib.LidarHipError, match="train mode"):
        model.train_loss(None, None, None)                           # eval mode
    model.train()
    for kw in ({"backbone": "folded"}, {"sparse": "nonsense"}, {"wgrad": "nonsense"}, {"deblock": "nonsense"},
               {"sparse": "fused", "backbone": "fused", "deblock": "wino"}):
        with pytest.raises(_lib.LidarHipError, match="must be"):
            model.train_loss(None, None, None, **kw)
    gen = DENSE_HEAD_CFG["ANCHOR_GENERATOR_CONFIG"]
    assert [c["feature_map_stride"] for c in gen] == [8, 8, 8]
    assert [(c["matched_threshold"], c["unmatched_threshold"]) for c in gen] == [(0.6, 0.45), (0.5, 0.35), (0.5, 0.35)]
    w = DENSE_HEAD_CFG["LOSS_CONFIG"]["LOSS_WEIGHTS"]
    assert w["loc_weight"] == 2.0 and w["dir_weight"] == 0.2 and model.grid == [1408, 1600, 40]
