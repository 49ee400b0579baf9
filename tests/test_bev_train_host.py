"""CPU checks of the train-mode BEV backbone (bev_train.py, csrc/bn_train.hip) before any kernel runs: the per-layer routing and its
fallbacks, the C ABI's pure-host workspace query and argument checks (nothing is launched: every call below is refused before a
launch), the mirror BaseBEVBackbone's state_dict keys against the reference fixture, and its reference-way forward off the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from lidardetection_amd import _lib, bev_train
from lidardetection_amd.pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
from lidardetection_amd.pointpillar import make_bev_backbone


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


FIXTURE_CFG = _Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[2, 2], NUM_FILTERS=[64, 32], UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[64, 64])


def _bn(c, **kw):
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01, **kw)


def test_bn_supported_predicate():
    assert bev_train.bn_supported(_bn(64))
    assert bev_train.bn_supported(_bn(4)) and bev_train.bn_supported(_bn(1024))
    assert not bev_train.bn_supported(_bn(6))                                  # C % 4 != 0
    assert not bev_train.bn_supported(_bn(2048))                               # wider than one block's row
    assert not bev_train.bn_supported(nn.BatchNorm2d(64, momentum=None))       # cumulative moving average
    assert not bev_train.bn_supported(_bn(64, affine=False))
    assert not bev_train.bn_supported(_bn(64, track_running_stats=False))
    assert not bev_train.bn_supported(nn.BatchNorm1d(64))
    assert not bev_train.bn_supported(_bn(64), channels=32)                    # the conv's width must be the norm's


def test_conv_routes_and_fallbacks():
    conv = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    assert bev_train.conv_route(conv, _bn(64)) == "wino"
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=0, bias=False), _bn(64), (1, 1, 1, 1)) == "wino"   # ZeroPad2d(1) + pad 0
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, stride=2, padding=0, bias=False), _bn(64), (1, 1, 1, 1)) == "conv"
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=1, bias=True), _bn(64)) == "conv"           # bias: stock conv
    assert bev_train.conv_route(nn.Conv2d(64, 64, 1, bias=False), _bn(64)) == "conv"
    assert bev_train.conv_route(nn.Conv2d(64, 40, 3, padding=1, bias=False), _bn(40)) == "conv"           # Winograd refuses Cout 40
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False), _bn(64)) == "stock"
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False), _bn(64)) == "stock"
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=0, bias=False), _bn(64), (1, 0, 1, 1)) == "stock"  # asymmetric pad
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=1, padding_mode="reflect", bias=False), _bn(64)) == "stock"
    assert bev_train.conv_route(nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64, momentum=None)) == "stock"
    assert bev_train.conv_route(nn.Conv2d(64, 6, 3, padding=1, bias=False), _bn(6)) == "stock"            # C % 4
    assert bev_train.wino_train_supported(64, 128) and bev_train.wino_train_supported(32, 32)
    assert not bev_train.wino_train_supported(16, 64)                          # the input gradient would have Cout 16


def test_backbone_plans_pointpillar_second_and_fixture():
    blocks, deblocks = make_bev_backbone()                                      # PointPillar-KITTI
    tb = bev_train.TrainBEVBackbone(blocks, deblocks)
    layers, de = tb.routes()
    assert layers == [["conv"] + ["wino"] * 3, ["conv"] + ["wino"] * 5, ["conv"] + ["wino"] * 5]
    assert de == ["fused"] * 3 and tb.de_merged and tb.extra is None
    blocks, deblocks = make_bev_backbone(cin=256, layer_nums=(5, 5), strides=(1, 2), filters=(128, 256), up_strides=(1, 2),
                                         up_filters=(256, 256))                 # SECOND: block 1 opens with a pad-1 stride-1 layer
    layers, de = bev_train.TrainBEVBackbone(blocks, deblocks).routes()
    assert layers == [["wino"] * 6, ["conv"] + ["wino"] * 5] and de == ["fused"] * 2
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    layers, de = bev_train.TrainBEVBackbone(m.blocks, m.deblocks).routes()
    assert layers == [["conv", "wino"], ["conv", "wino"]] and de == ["fused", "fused"]


def test_backbone_plan_falls_back_per_layer():
    blocks, deblocks = make_bev_backbone(cin=64, layer_nums=(2,), strides=(2,), filters=(64,), up_strides=(1,), up_filters=(128,))
    blocks[0][5] = nn.BatchNorm2d(64, eps=1e-3, momentum=None)                 # second layer's norm: cumulative average
    deblocks[0][1].momentum = None
    tb = bev_train.TrainBEVBackbone(blocks, deblocks)
    layers, de = tb.routes()
    assert layers == [["conv", "stock", "wino"]] and de == ["stock"] and not tb.de_merged
    odd = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1), nn.ReLU())             # not Conv / BN / ReLU triplets: the whole block stock
    assert bev_train.TrainBEVBackbone([odd], []).routes() == ([["stock"]], [])


def test_workspace_query_is_pure_host():
    L = _lib.lib()
    rows = 16 * 248 * 216
    assert L.lidar_bn_relu_train_workspace_bytes(rows, 64) >= 2 * 64 * 8
    assert L.lidar_bn_relu_train_workspace_bytes(rows, 384) > L.lidar_bn_relu_train_workspace_bytes(rows, 64)
    assert L.lidar_bn_relu_train_workspace_bytes(0, 64) == 0 and L.lidar_bn_relu_train_workspace_bytes(10, 0) == 0
    assert L.lidar_bn_relu_train_workspace_bytes(2, 4) % 256 == 0


def _fwd(L, nseg=1, ptr=0x10000, ld=64, off=0, c=64, rows=100, y_ld=64, y_off=0, ws_bytes=1 << 30, eps=1e-3):
    """lidar_bn_relu_train_forward with fake (never dereferenced) aligned addresses: every case here is refused before a launch"""
    n = max(nseg, 1)
    xs = (C.c_void_p * n)(*([ptr] * n))
    a = C.c_void_p(0x20000)
    return L.lidar_bn_relu_train_forward(nseg, xs, _lib.host_i32([ld] * n), _lib.host_i32([off] * n), _lib.host_i32([c] * n), rows,
                                         a, a, eps, a, y_ld, y_off, a, a, a, a, ws_bytes, None)


def test_argument_errors_return_status_not_exit():
    L = _lib.lib()
    assert _fwd(L, nseg=0) == -1 and _fwd(L, nseg=5) == -1          # 1..4 inputs per call
    assert _fwd(L, c=6, ld=8) == -1                                   # C % 4
    assert _fwd(L, c=2048, ld=2048) == -1                             # wider than BT_MAX_C
    assert _fwd(L, ptr=0x10004) == -1                                 # a 16-byte misaligned map
    assert _fwd(L, off=4) == -1                                       # off + C > ld
    assert _fwd(L, ld=66, c=64) == -1                                 # ld % 4
    assert _fwd(L, rows=1) == -1                                      # N = 1: torch refuses it too
    assert _fwd(L, y_ld=32) == -1                                     # the output cannot hold the channels
    assert _fwd(L, eps=float("nan")) == -1
    assert _fwd(L, ws_bytes=16) == -3                                 # LIDAR_ERR_WORKSPACE
    xs = (C.c_void_p * 1)(0x10000)
    one = _lib.host_i32([64])
    a = C.c_void_p(0x20000)
    assert L.lidar_bn_relu_train_backward(1, xs, one, _lib.host_i32([0]), one, 100, a, 64, 0, a, a, a, None, a, a, a, 1 << 30,
                                          None) == -1                  # no dz table
    assert L.lidar_bn_relu_train_backward(1, xs, one, _lib.host_i32([0]), one, 1, a, 64, 0, a, a, a, xs, a, a, a, 1 << 30, None) == -1


def test_python_layer_refuses_what_the_kernels_do_not_take():
    bn = _bn(64)
    with pytest.raises(_lib.LidarHipError):
        bev_train.bn_relu_train(torch.zeros(2, 64, 4, 4), nn.BatchNorm2d(64, momentum=None))
    with pytest.raises(_lib.LidarHipError):
        bev_train.bn_relu_train([torch.zeros(2, 64, 4, 4)], [bn, bn])
    with pytest.raises(_lib.LidarHipError):             # CPU map: no CPU path
        bev_train.TrainBEVBackbone(*make_bev_backbone(layer_nums=(1,), strides=(2,), filters=(64,), up_strides=(1,),
                                                      up_filters=(64,)))(torch.zeros(2, 64, 8, 8))


def test_mirror_state_dict_keys_match_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "bev_train_ref.npz"))
    keys = sorted(k[4:] for k in z.files if k.startswith("bev."))
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    assert sorted(m.state_dict().keys()) == keys
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == z["bev." + k].shape, k
    assert m.num_bev_features == 128


def test_mirror_off_gpu_is_the_reference_computation():
    torch.manual_seed(0)
    m = BaseBEVBackbone(FIXTURE_CFG, 16).train()
    ref = BaseBEVBackbone(FIXTURE_CFG, 16).train()
    ref.load_state_dict(m.state_dict())
    x = torch.randn(2, 16, 16, 16)
    y = m({"spatial_features": x})["spatial_features_2d"]
    ups, h = [], x
    for blk, de in zip(ref.blocks, ref.deblocks):
        h = blk(h)
        ups.append(de(h))
    torch.testing.assert_close(y, torch.cat(ups, 1), rtol=0, atol=0)
    assert int(m.blocks[0][2].num_batches_tracked) == 1
    frac = BaseBEVBackbone(_Cfg(LAYER_NUMS=[1], LAYER_STRIDES=[2], NUM_FILTERS=[32], UPSAMPLE_STRIDES=[0.5], NUM_UPSAMPLE_FILTERS=[32]), 16)
    assert isinstance(frac.deblocks[0][0], nn.Conv2d) and tuple(frac.deblocks[0][0].stride) == (2, 2)
