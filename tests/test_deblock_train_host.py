"""Host-side checks (no GPU) of the deblock training path: the pure-host C ABI queries of csrc/deconv_train.hip over the edges of their
declared range, status codes instead of launches for bad arguments, the deblock option of bev_train / pointpillar (routes, argument
errors), and the reference fixture tests/golden/deblock_train_ref.npz replayed in float64 on this repo's module tree."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from _gpu_util import rel
from lidardetection_amd import _lib, bev_train
from lidardetection_amd.pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
from lidardetection_amd.pointpillar import make_bev_backbone


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


FIXTURE_CFG = _Cfg(LAYER_NUMS=[0, 0, 0], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=[16, 24, 24], UPSAMPLE_STRIDES=[1, 2, 4],
                   NUM_UPSAMPLE_FILTERS=[128, 128, 128])
LIB3 = ("library", "library", "library")


def _declared_range():
    """LIDAR_DECONV_TRAIN_* as include/lidar_hip.h declares them"""
    return {k[len("LIDAR_DECONV_TRAIN_"):]: v for k, v in _lib.LIMITS.items() if k.startswith("LIDAR_DECONV_TRAIN_")}


def test_supported_range_edges():
    L = _lib.lib()
    r = _declared_range()
    assert r == {"MIN_K": 16, "MIN_CUP": 32, "MAX_C": 512}
    ok = L.lidar_deconv_train_supported
    for K, s, c_up in [(64, 1, 128), (128, 2, 128), (256, 4, 128), (128, 1, 256), (256, 2, 256)]:      # every deblock the repo builds
        assert ok(K, s, c_up) == 1 and bev_train.deconv_train_supported(K, s, c_up)
    # K: just inside and just outside
    assert ok(16, 2, 128) == 1 and ok(24, 2, 128) == 1 and ok(512, 2, 128) == 1
    assert ok(8, 2, 128) == 0 and ok(20, 2, 128) == 0 and ok(520, 2, 128) == 0 and ok(0, 2, 128) == 0 and ok(-16, 2, 128) == 0
    # C_up
    assert ok(64, 2, 32) == 1 and ok(64, 2, 96) == 1 and ok(64, 2, 512) == 1
    assert ok(64, 2, 16) == 0 and ok(64, 2, 48) == 0 and ok(64, 2, 544) == 0 and ok(64, 2, 0) == 0
    # s
    assert ok(64, 1, 128) == 1 and ok(64, 2, 128) == 1 and ok(64, 4, 128) == 1
    assert ok(64, 0, 128) == 0 and ok(64, 3, 128) == 0 and ok(64, 8, 128) == 0 and ok(64, -1, 128) == 0
    assert not bev_train.deconv_train_supported(64, 3, 128)


def test_workspace_bytes_is_pure_host():
    L = _lib.lib()
    q = L.lidar_deconv_wgrad_workspace_bytes
    for shape in [(16, 248, 216, 64, 1, 128), (16, 124, 108, 128, 2, 128), (16, 62, 54, 256, 4, 128), (1, 1, 1, 16, 1, 32)]:
        B, h, w, K, s, c_up = shape
        n = q(*shape)
        per_split = K * s * s * c_up * 4
        assert n > 0 and n % per_split == 0 and n == q(*shape), shape
        splits = n // per_split
        assert -(-B * h * w // splits) <= 4096 + 32, shape              # no fp32 accumulation runs over more than ~4096 pixels
    assert q(1, 1, 1, 16, 1, 32) == 16 * 32 * 4                         # one pixel: one partial
    for shape in [(0, 8, 8, 64, 2, 128), (2, 0, 8, 64, 2, 128), (2, 8, -1, 64, 2, 128), (2, 8, 8, 20, 2, 128), (2, 8, 8, 64, 3, 128),
                  (2, 8, 8, 64, 2, 48), (2, 8, 8, 1024, 2, 128)]:
        assert q(*shape) == 0, shape


def test_bad_arguments_return_a_status():
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.float32)                        # host memory: every call below returns before any launch
    assert buf.data_ptr() % 16 == 0
    p = _lib.ptr(buf)
    off4 = _lib.C.c_void_p(buf.data_ptr() + 4)
    big = 1 << 30

    def dgrad(g=p, g_ld=128, W=p, B=1, h=4, w=4, K=64, s=2, c_up=128, dx=p, dx_ld=64):
        return L.lidar_deconv_dgrad_nhwc(g, g_ld, W, B, h, w, K, s, c_up, dx, dx_ld, None)

    def wgrad(x=p, x_ld=64, g=p, g_ld=128, B=1, h=4, w=4, K=64, s=2, c_up=128, dw=p, ws=p, wsb=big):
        return L.lidar_deconv_wgrad_nhwc(x, x_ld, g, g_ld, B, h, w, K, s, c_up, dw, ws, wsb, None)

    assert dgrad(g=None) == -1 and dgrad(W=None) == -1 and dgrad(dx=None) == -1
    assert wgrad(x=None) == -1 and wgrad(g=None) == -1 and wgrad(dw=None) == -1
    assert dgrad(g_ld=96) == -1 and dgrad(dx_ld=56) == -1              # row stride shorter than the channels
    assert wgrad(x_ld=56) == -1 and wgrad(g_ld=124) == -1
    assert dgrad(g_ld=130) == -1 and wgrad(x_ld=66) == -1 and wgrad(g_ld=130) == -1      # row stride no multiple of 4 floats
    assert dgrad(g=off4) == -1 and wgrad(x=off4) == -1 and wgrad(g=off4) == -1           # misaligned maps
    for bad in (dict(K=20, dx_ld=64), dict(K=1024, dx_ld=1024), dict(s=3), dict(c_up=48), dict(c_up=1024, g_ld=1024)):
        assert dgrad(**bad) == -1, bad
    for bad in (dict(K=20), dict(K=1024, x_ld=1024), dict(s=3), dict(c_up=48), dict(c_up=1024, g_ld=1024)):
        assert wgrad(**bad) == -1, bad
    assert dgrad(B=0) == -1 and dgrad(h=0) == -1 and dgrad(w=-3) == -1 and wgrad(B=0) == -1 and wgrad(h=-1) == -1 and wgrad(w=0) == -1
    # maps at the byte limit.  s = 1, 128 floats per gradient pixel: 2^22 pixels are exactly 2^31 bytes, one row of pixels fewer fits
    assert dgrad(B=4, h=1024, w=1024, s=1, g_ld=128, dx_ld=64) == -1 and wgrad(B=4, h=1024, w=1024, s=1, g_ld=128) == -1
    assert dgrad(B=8, h=1024, w=1024, s=1, g_ld=32, c_up=32, K=16, dx_ld=64) == -1      # dx alone: 2^31 bytes
    assert wgrad(B=2, h=1024, w=1024, s=2, g_ld=128) == -1                               # the upsampled gradient map: 2^31 bytes
    assert wgrad(B=8, h=1024, w=1024, s=1, x_ld=64, g_ld=32, c_up=32) == -1              # x alone
    # a workspace that is missing, misaligned or one byte short
    need = L.lidar_deconv_wgrad_workspace_bytes(1, 4, 4, 64, 2, 128)
    assert need > 0
    assert wgrad(ws=None) == -3 and wgrad(ws=off4) == -3 and wgrad(wsb=need - 1) == -3 and wgrad(wsb=0) == -3


def test_fits_is_host_arithmetic():
    fits = bev_train.deconv_train_fits
    assert fits(16, 248, 216, 1, 64, 128) and fits(16, 62, 54, 4, 256, 128)
    assert not fits(4, 1024, 1024, 1, 64, 128) and fits(4, 1024, 1023, 1, 64, 128)
    assert not fits(2, 1024, 1024, 2, 64, 128)                         # the upsampled map is the large one
    assert not fits(0, 8, 8, 2, 64, 128) and not fits(2, 8, 8, 2, 66, 128) and not fits(2, 8, 8, 2, 64, 130)
    E = _lib.LidarHipError
    x, g, w = torch.zeros(1, 64, 4, 4), torch.zeros(1, 128, 8, 8), torch.zeros(64, 128, 2, 2)
    cl = torch.channels_last
    for fn, args in ((bev_train.deconv_wgrad, (x.contiguous(memory_format=cl), g.contiguous(memory_format=cl), 2)),
                     (bev_train.deconv_dgrad, (g.contiguous(memory_format=cl), w, 2)),
                     (bev_train.deconv_train, (x.contiguous(memory_format=cl), w, 2, "gemm"))):
        with pytest.raises(E):                                          # CPU tensors: no CPU path
            fn(*args)


def _second():
    return make_bev_backbone(cin=256, layer_nums=(5, 5), strides=(1, 2), filters=(128, 256), up_strides=(1, 2), up_filters=(256, 256))


def test_deblock_conv_routes():
    route = bev_train.deblock_conv_route
    pp = make_bev_backbone()
    lib, new = bev_train.TrainBEVBackbone(*pp), bev_train.TrainBEVBackbone(*pp, wgrad="wino", deblock="gemm")
    assert lib.deblock_conv_routes() == [LIB3] * 3
    # PointPillar: 64 -> 128 s = 1 (the forward kernel needs s^2 C_up % 512 == 0), 128 -> 128 s = 2, 256 -> 128 s = 4
    assert new.deblock_conv_routes() == [("library", "gemm", "gemm"), ("gemm", "gemm", "gemm"), ("gemm", "gemm", "gemm")]
    assert [route(de, "gemm") for de in pp[1]] == new.deblock_conv_routes() and [route(de) for de in pp[1]] == [LIB3] * 3
    # the other routes and their return values are what they were
    assert lib.routes() == new.routes() == ([["conv"] + ["wino"] * 3, ["conv"] + ["wino"] * 5, ["conv"] + ["wino"] * 5], ["fused"] * 3)
    assert new.wgrad_routes() == bev_train.TrainBEVBackbone(*pp, wgrad="wino").wgrad_routes()
    assert bev_train.TrainBEVBackbone(pp[0], pp[1], "library", "gemm").wgrad_routes() == lib.wgrad_routes()
    sec = _second()                                                    # SECOND: 128 -> 256 s = 1 (256 % 512 != 0), 256 -> 256 s = 2
    new = bev_train.TrainBEVBackbone(*sec, deblock="gemm")
    assert new.deblock_conv_routes() == [("library", "gemm", "gemm"), ("gemm", "gemm", "gemm")]
    assert new.routes() == bev_train.TrainBEVBackbone(*sec).routes() == ([["wino"] * 6, ["conv"] + ["wino"] * 5], ["fused"] * 2)

    def de(up, c=128):
        return nn.Sequential(up, nn.BatchNorm2d(c, eps=1e-3, momentum=0.01), nn.ReLU())

    assert route(de(nn.ConvTranspose2d(64, 128, 2, stride=2, bias=False)), "gemm") == ("gemm", "gemm", "gemm")
    assert route(de(nn.Conv2d(64, 128, 2, stride=2, bias=False)), "gemm") == LIB3                  # UPSAMPLE_STRIDE < 1
    assert route(de(nn.ConvTranspose2d(64, 128, 2, stride=2, bias=True)), "gemm") == LIB3           # biased
    assert route(de(nn.ConvTranspose2d(64, 128, 3, stride=2, padding=1, bias=False)), "gemm") == LIB3
    assert route(de(nn.ConvTranspose2d(64, 128, 4, stride=2, bias=False)), "gemm") == LIB3          # kernel != stride
    assert route(de(nn.ConvTranspose2d(64, 128, 3, stride=3, bias=False)), "gemm") == LIB3          # s = 3
    assert route(de(nn.ConvTranspose2d(64, 128, 2, stride=2, groups=2, bias=False)), "gemm") == LIB3
    assert route(de(nn.ConvTranspose2d(20, 128, 2, stride=2, bias=False)), "gemm") == LIB3          # K % 8
    assert route(de(nn.ConvTranspose2d(64, 48, 2, stride=2, bias=False), 48), "gemm") == LIB3       # C_up % 32
    assert route(de(nn.ConvTranspose2d(64, 96, 2, stride=2, bias=False), 96), "gemm") == ("library", "gemm", "gemm")   # C_up % 128
    frac = BaseBEVBackbone(_Cfg(LAYER_NUMS=[1], LAYER_STRIDES=[2], NUM_FILTERS=[32], UPSAMPLE_STRIDES=[0.5], NUM_UPSAMPLE_FILTERS=[32]), 16)
    assert bev_train.TrainBEVBackbone(frac.blocks, frac.deblocks, deblock="gemm").deblock_conv_routes() == [LIB3]
    # a deblock the backbone runs as the stock module keeps the library for its up-convolution too
    blocks, deblocks = make_bev_backbone(cin=64, layer_nums=(1,), strides=(2,), filters=(64,), up_strides=(2,), up_filters=(128,))
    deblocks[0][1].momentum = None
    tb = bev_train.TrainBEVBackbone(blocks, deblocks, deblock="gemm")
    assert tb.routes()[1] == ["stock"] and tb.deblock_conv_routes() == [LIB3]
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    tb = bev_train.TrainBEVBackbone(m.blocks, m.deblocks, deblock="gemm")
    assert tb.deblock_conv_routes() == [("library", "gemm", "gemm"), ("gemm", "gemm", "gemm"), ("gemm", "gemm", "gemm")]
    assert tb.routes() == ([["conv"], ["conv"], ["conv"]], ["fused"] * 3) and tb.de_merged


def test_unknown_option_raises_at_every_level():
    from lidardetection_amd.pointpillar import PointPillarKITTI
    E = _lib.LidarHipError
    pp = make_bev_backbone()
    assert bev_train.DEBLOCK_OPTIONS == ("library", "gemm")
    with pytest.raises(E):
        bev_train.TrainBEVBackbone(*pp, deblock="nonsense")
    with pytest.raises(E):
        bev_train.TrainBEVBackbone(*pp, deblock="wino")
    with pytest.raises(E):
        bev_train.deconv_train(torch.zeros(1, 64, 4, 4), torch.zeros(64, 128, 2, 2), 2, deblock="nonsense")
    with pytest.raises(E):
        bev_train.deblock_conv_route(pp[1][0], "nonsense")
    # the model's methods check the option before they touch the device
    for fn, args in ((PointPillarKITTI.backbone_head_train, (None,)), (PointPillarKITTI.train_loss, (None, None, None))):
        class _Stub:
            training, channels_last = True, True
        with pytest.raises(E):
            fn(_Stub(), *args, deblock="nonsense")
        with pytest.raises(E):
            fn(_Stub(), *args, wgrad="wino", deblock="wino")


def _fixture_model(z):
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    sd = {}
    for k, v in m.state_dict().items():
        a = torch.from_numpy(z["bev." + k])
        sd[k] = a.float() * float(z["weight_scale"]) if a.dtype == torch.int8 else a
    m.load_state_dict(sd)
    return m


def test_fixture_keys_and_float64_replay(golden_dir):
    """the fixture is consistent with itself: this repo's module tree (stock modules, float64, CPU) run on the stored inputs gives the
    stored output and gradients"""
    path = os.path.join(golden_dir, "deblock_train_ref.npz")
    assert os.path.getsize(path) <= 351428                              # the largest fixture before this one
    z = np.load(path)
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    assert sorted(m.state_dict().keys()) == sorted(k[4:] for k in z.files if k.startswith("bev."))
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == z["bev." + k].shape, k
    assert m.num_bev_features == 384
    m = _fixture_model(z).double().train()
    x = (torch.from_numpy(z["x_code"]).double() * float(z["x_scale"])).requires_grad_()
    G = torch.from_numpy(z["g_code"]).double() * float(z["g_scale"])
    assert tuple(x.shape) == (2, 16, 8, 4) and tuple(G.shape) == (2, 384, 8, 4)
    y = m({"spatial_features": x})["spatial_features_2d"]
    assert rel(y, torch.from_numpy(z["out64"])) < 2.0 ** -22           # stored rounded to float32
    (y * G).sum().backward()
    assert rel(x.grad, torch.from_numpy(z["dx64"])) < 2.0 ** -22
    n_up = 0
    for name, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            assert rel(mod.weight.grad, torch.from_numpy(z["d_gamma." + name])) < 2.0 ** -22, name
            assert rel(mod.bias.grad, torch.from_numpy(z["d_beta." + name])) < 2.0 ** -22, name
            assert rel(mod.running_mean, torch.from_numpy(z["rm1." + name])) < 2.0 ** -22, name
            assert rel(mod.running_var, torch.from_numpy(z["rv1." + name])) < 2.0 ** -22, name
        elif isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            key = name + ".weight"
            ref = torch.from_numpy(z["dw16." + key].astype(np.float64)) * float(z["dw_scale." + key])
            assert rel(mod.weight.grad, ref) < 2.0 ** -10, name          # float16 storage: 11 significant bits of the largest value
            n_up += isinstance(mod, nn.ConvTranspose2d)
    assert n_up == 3
