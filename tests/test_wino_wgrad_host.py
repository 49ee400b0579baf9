"""Host-side checks (no GPU) of the Winograd weight-gradient path: the pure-host C ABI queries of csrc/wino43_wgrad.hip, status codes
instead of exits for bad arguments, and the wgrad option of bev_train / pointpillar (routes, argument errors)."""
import pytest
import torch

from lidardetection_amd import _lib, bev_train, wino
from lidardetection_amd.pointpillar import make_bev_backbone

WS_BLOCK = 36 * 32 * 32 * 4        # bytes of one workgroup's partial: 36 positions x 32 co x 32 ci floats


def test_supported_widths():
    L = _lib.lib()
    for c in (32, 64, 128, 256, 512):
        assert L.lidar_wino43_wgrad_supported(c, c) == 1 and wino.wgrad43_supported(c, c)
    assert L.lidar_wino43_wgrad_supported(64, 128) == 1 and L.lidar_wino43_wgrad_supported(256, 32) == 1
    for cin, cout in [(0, 64), (64, 0), (-32, 64), (16, 64), (64, 48), (96 + 8, 64), (1024, 1024), (64, 544)]:
        assert L.lidar_wino43_wgrad_supported(cin, cout) == 0, (cin, cout)
        assert not wino.wgrad43_supported(cin, cout)


def test_workspace_bytes_is_pure_host():
    L = _lib.lib()
    for shape in [(16, 248, 216, 64, 64), (16, 124, 108, 128, 128), (16, 62, 54, 256, 256), (1, 3, 2, 64, 64), (2, 5, 1, 128, 128)]:
        n = L.lidar_wino43_wgrad_workspace_bytes(*shape)
        assert n > 0 and n % WS_BLOCK == 0, shape
        B, H, W, cin, cout = shape
        tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
        splits = n // WS_BLOCK // ((cin // 32) * (cout // 32))
        assert splits >= 1 and -(-tiles // splits) <= 512 + 8         # no fp32 accumulation runs over more than ~512 tiles
        assert n == L.lidar_wino43_wgrad_workspace_bytes(*shape)
    assert L.lidar_wino43_wgrad_workspace_bytes(1, 3, 2, 64, 64) == 4 * WS_BLOCK     # one tile: one split of each of the 4 blocks
    for shape in [(0, 8, 8, 64, 64), (2, 0, 8, 64, 64), (2, 8, 0, 64, 64), (-1, 8, 8, 64, 64), (2, 8, 8, 48, 64), (2, 8, 8, 64, 1024)]:
        assert L.lidar_wino43_wgrad_workspace_bytes(*shape) == 0, shape


def test_bad_arguments_return_a_status():
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.float32)                      # host memory: every call below returns before any launch
    p = _lib.ptr(buf)
    big = 1 << 20

    def call(x=p, x_ld=64, g=p, g_ld=64, B=1, H=4, W=4, cin=64, cout=64, dw=p, ws=p, wsb=big):
        return L.lidar_wino43_wgrad_nhwc(x, x_ld, g, g_ld, B, H, W, cin, cout, dw, ws, wsb, None)

    assert call(x=None) == -1 and call(g=None) == -1 and call(dw=None) == -1
    assert call(cin=48) == -1 and call(cout=1024, g_ld=1024) == -1
    assert call(x_ld=32) == -1 and call(g_ld=63) == -1               # row stride shorter than the channels
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=-3) == -1
    assert call(B=16, H=1024, W=1024, x_ld=64) == -1                 # 2^32 bytes: beyond the 32-bit offsets
    assert call(B=8, H=1024, W=1024, x_ld=64, g_ld=64) == -1         # exactly 2^31 bytes
    assert call(ws=None) == -3 and call(wsb=WS_BLOCK * 4 - 1) == -3  # missing / short workspace


def test_fits_is_host_arithmetic():
    assert wino.wgrad43_fits((16, 64, 248, 216), 64)
    assert not wino.wgrad43_fits((8, 64, 1024, 1024), 64)            # 2^31 bytes
    assert not wino.wgrad43_fits((8, 32, 1024, 1024), 64)            # the gradient map is the large one
    assert wino.wgrad43_fits((8, 32, 1024, 1024), 32) and not wino.wgrad43_fits((8, 32, 1024, 1024), 32, x_ld=64)
    assert not wino.wgrad43_fits((0, 64, 8, 8), 64)
    with pytest.raises(_lib.LidarHipError):
        wino.conv3x3_wgrad_f43(torch.zeros(1, 64, 4, 4), torch.zeros(1, 64, 4, 4))     # CPU tensors: no CPU path


def _second():
    return make_bev_backbone(cin=256, layer_nums=(5, 5), strides=(1, 2), filters=(128, 256), up_strides=(1, 2), up_filters=(256, 256))


def test_wgrad_routes():
    pp = make_bev_backbone()
    lib, new = bev_train.TrainBEVBackbone(*pp), bev_train.TrainBEVBackbone(*pp, wgrad="wino")
    assert lib.routes() == new.routes() == bev_train.TrainBEVBackbone(pp[0], pp[1], "library").routes()
    assert new.wgrad_routes() == [[None] + ["wino"] * 3, [None] + ["wino"] * 5, [None] + ["wino"] * 5]
    assert lib.wgrad_routes() == [[None] + ["library"] * 3, [None] + ["library"] * 5, [None] + ["library"] * 5]
    sec = _second()
    new = bev_train.TrainBEVBackbone(*sec, wgrad="wino")
    assert new.routes() == bev_train.TrainBEVBackbone(*sec).routes()
    # SECOND: block 1's first layer is a stride-1 256 -> 128 layer on the Winograd route; block 2's first layer has stride 2
    assert new.wgrad_routes() == [["wino"] * 6, [None] + ["wino"] * 5]
    # one width the weight-gradient kernel does not take (1024 > 512): those layers stay on the library, the others do not
    odd = make_bev_backbone(cin=64, layer_nums=(2, 2), strides=(2, 2), filters=(64, 1024), up_strides=(1, 2), up_filters=(64, 64))
    new = bev_train.TrainBEVBackbone(*odd, wgrad="wino")
    assert new.routes()[0] == [["conv", "wino", "wino"], ["conv", "wino", "wino"]]
    assert new.wgrad_routes() == [[None, "wino", "wino"], [None, "library", "library"]]
    assert bev_train.wgrad_route(64, 64, "wino") == "wino" and bev_train.wgrad_route(64, 64) == "library"
    assert bev_train.wgrad_route(1024, 1024, "wino") == "library"


def test_unknown_option_raises_at_every_level():
    from lidardetection_amd.pointpillar import PointPillarKITTI
    E = _lib.LidarHipError
    pp = make_bev_backbone()
    with pytest.raises(E):
        bev_train.TrainBEVBackbone(*pp, wgrad="nonsense")
    with pytest.raises(E):
        bev_train.conv3x3_train(torch.zeros(1, 64, 4, 4), torch.zeros(64, 64, 3, 3), wgrad="nonsense")
    with pytest.raises(E):
        bev_train.wgrad_route(64, 64, "nonsense")
    assert "wgrad" in PointPillarKITTI.train_loss.__code__.co_varnames and "wgrad" in PointPillarKITTI.backbone_head_train.__code__.co_varnames
    # the model's methods check the option before they touch the device
    for fn, args in ((PointPillarKITTI.backbone_head_train, (None,)), (PointPillarKITTI.train_loss, (None, None, None))):
        class _Stub:
            training, channels_last = True, True
        with pytest.raises(E):
            fn(_Stub(), *args, wgrad="nonsense")
