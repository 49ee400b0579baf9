"""The shared-transform workgroup shape of the F(4x4, 3x3) kernel (csrc/wino43_conv.hip: wino_f43s_kernel, one tile group x four
blocks of 32 output channels, for Cout % 128 == 0) against the shape it replaces on those layers (two tile groups x two blocks).
Per output element the K order of the accumulation, the transform expressions and the epilogue are the same, so the results must be
EQUAL BIT FOR BIT; and within 1e-4 x max(1, |ref|max) of torch.nn.functional.conv2d in float64 (the kernel's existing bound).
The last test is host-only (no `gpu` mark): the supported / packed-size entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lidardetection_amd import _lib, wino

CL = torch.channels_last


def _ref(x, w, bias, relu):
    y = F.conv2d(x.double().cpu(), w.double().cpu(), None if bias is None else bias.double().cpu(), 1, 1)
    return torch.relu(y) if relu else y


def _form(H, W):
    """the tile-group form lidar_wino43s_conv3x3_nhwc picks: fewest groups of 4 x 4, 2 x 8, 8 x 2 tiles, first on a tie"""
    ty, tx = (H + 3) // 4, (W + 3) // 4
    n = [-(-ty // a) * -(-tx // b) for a, b in ((4, 4), (2, 8), (8, 2))]
    return ("4x4", "2x8", "8x2")[n.index(min(n))]


def _data(B, cin, cout, H, W, in_c):
    g = torch.Generator(device="cpu").manual_seed(1000 * cin + cout + 7 * H + W)
    x = torch.randn(B, in_c, H, W, generator=g)
    x[:, :, 0, :] += 2.0                                    # make the borders matter (zero padding must really be zero)
    x[:, :, :, -1] -= 3.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g)
    return x, w, bias


# (B, Cin, Cout, H, W), the tile-group form the shared shape runs it on
SHAPES = [
    ((1, 32, 128, 5, 7), "4x4"),        # partial tiles and halo: one group, most of it outside the map
    ((2, 128, 256, 9, 13), "4x4"),      # two workgroups along Cout, 16 chunks
    ((1, 32, 384, 17, 6), "8x2"),       # three workgroups along Cout, a map narrower than a 2 x 8 tile group
    ((2, 48, 128, 30, 29), "4x4"),      # 2 x 2 groups of 4 x 4 tiles per frame, partial at both edges; Cin not a multiple of 32
    ((1, 32, 128, 6, 40), "2x8"),       # 2 x 8 tiles, two groups along x
    ((1, 64, 128, 62, 54), "8x2"),      # 8 x 2 tiles (PointPillar block 3 geometry), 2 x 7 groups
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,form", SHAPES)
def test_share_shape_equals_the_two_group_shape_bit_for_bit(dev, shape, form):
    """each shape: through an input map of channel pitch in_C > Cin and into a channel slice of a wider output map (neighbouring
    channels bit-unchanged); with and without ReLU and bias; two calls give the same bits; equal bits with the two-group shape;
    |error| <= 1e-4 max(1, |ref|max) against the float64 convolution"""
    B, cin, cout, H, W = shape
    assert _form(H, W) == form
    in_c, out_c, off = cin + 8, cout + 48, 16
    x, w, bias = _data(B, cin, cout, H, W, in_c)
    xd, wd, bd = x.to(dev).contiguous(memory_format=CL), w.to(dev), bias.to(dev)
    p_old, p_new = wino.pack_weights43(wd), wino.pack_weights43_share(wd)
    assert p_old.numel() == p_new.numel() == 36 * cin * cout
    assert torch.equal(p_new.sort().values, p_old.sort().values)          # the same filters in another order
    for relu, b in ((True, bd), (False, None), (False, bd)):
        outs = []
        for packed, share in ((p_old, False), (p_new, True), (p_new, True)):
            out = torch.full((B, out_c, H, W), 7.0, device=dev).contiguous(memory_format=CL)
            wino.conv3x3_f43(xd, packed, cout, b, relu, out=out, out_offset=off, cin=cin, share=share)
            assert bool((out[:, :off] == 7.0).all()) and bool((out[:, off + cout:] == 7.0).all())
            outs.append(out[:, off:off + cout])
        want = _ref(x[:, :cin], w, None if b is None else bias, relu)
        scale = max(1.0, float(want.abs().max()))
        err = float((outs[1].double().cpu() - want).abs().max())
        print(f"f43 share {shape} relu {relu} bias {b is not None}: max err {err:.2e} (scale {scale:.1f})")
        assert torch.equal(outs[1], outs[2]), "two calls differ"
        assert torch.equal(outs[1], outs[0]), "differs from the two-group shape"
        assert err <= 1e-4 * scale, (err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 16, 128, 5, 7), (1, 32, 128, 5, 7), (2, 128, 256, 9, 13), (1, 32, 384, 17, 6), (1, 64, 64, 9, 13)])
def test_routing_share_on_and_off_gives_the_same_bits(dev, monkeypatch, shape):
    """pack_auto / conv3x3_auto with LIDAR_WINO43_SHARE routing on and off (wino._F43_SHARE): the shared layout exactly where
    Cout % 128 == 0 and the F(4x4) kernel takes the layer, equal bits, within 1e-4 of float64.  (1, 16, 128, 5, 7): Cin = 16 is below
    what the F(4x4) kernel takes in either shape (Cin >= 32), both routings run F(2x2); (1, 64, 64, ...): 64 channels keep the
    two-group shape."""
    B, cin, cout, H, W = shape
    x, w, bias = _data(B, cin, cout, H, W, cin)
    xd, wd, bd = x.to(dev).contiguous(memory_format=CL), w.to(dev), bias.to(dev)
    got = {}
    for share in (False, True):
        monkeypatch.setattr(wino, "_F43_SHARE", [share])
        packed = wino.pack_auto(wd)
        marked = bool(getattr(packed[1], "w43_share", False))
        assert marked == (share and packed[0] == "f43" and cout % 128 == 0), (shape, share)
        assert (packed[0] == "f43") == (cin >= 32)
        out = torch.full((B, cout + 32, H, W), -5.0, device=dev).contiguous(memory_format=CL)
        wino.conv3x3_auto(xd, packed, cout, bd, True, out=out, out_offset=32)
        assert bool((out[:, :32] == -5.0).all())
        got[share] = (out[:, 32:], wino.conv3x3_auto(xd, packed, cout, None, False))
    want = (_ref(x, w, bias, True), _ref(x, w, None, False))
    for k in (0, 1):
        assert torch.equal(got[True][k], got[False][k])
        assert float((got[True][k].double().cpu() - want[k]).abs().max()) <= 1e-4 * max(1.0, float(want[k].abs().max()))
    if cout % 128 == 0 and cin >= 32:                       # the layouts must not be mixed up
        with pytest.raises(_lib.LidarHipError):
            wino.conv3x3_f43(xd, wino.pack_weights43(wd), cout, bd, True, share=True)
        with pytest.raises(_lib.LidarHipError):
            wino.conv3x3_f43(xd, wino.pack_weights43_share(wd), cout, bd, True)


@pytest.mark.gpu
def test_share_shape_walks_several_blocks_per_workgroup(dev):
    """70 frames of 32 x 32 = 280 tile groups: more blocks than workgroups (one per CU), so workgroups walk on to a next block and the
    input stream crosses blocks mid-pipeline with the fewest chunks per block (Cin = 32: four)"""
    B, cin, cout, H, W = 70, 32, 128, 32, 32
    x, w, bias = _data(B, cin, cout, H, W, cin)
    xd, wd, bd = x.to(dev).contiguous(memory_format=CL), w.to(dev), bias.to(dev)
    new = wino.conv3x3_f43(xd, wino.pack_weights43_share(wd), cout, bd, True, share=True)
    old = wino.conv3x3_f43(xd, wino.pack_weights43(wd), cout, bd, True)
    want = _ref(x, w, bias, True)
    assert torch.equal(new, old)
    assert float((new.double().cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_share_entry_points_refuse_what_the_kernel_does_not_take():
    """host only: Cout % 128 != 0, Cin % 16 != 0, Cin < 32 are refused by the supported / packed-size / pack / launch entry points
    (before anything is launched: the addresses are fake); the size is the 36 Cin Cout floats wino43s_pack_kernel writes, the same
    count as the two-group layout"""
    import ctypes as C
    L = _lib.lib()
    a = C.c_void_p(0x20000)
    for cin, cout in ((32, 64), (32, 192), (32, 320), (32, 0), (32, -128), (40, 128), (24, 128), (16, 128), (0, 128), (-32, 128), (72, 256)):
        assert not L.lidar_wino43s_supported(cin, cout) and L.lidar_wino43s_packed_floats(cin, cout) == 0, (cin, cout)
        assert not wino.supported43_share(cin, cout)
        assert L.lidar_wino43s_pack_weights(a, cin, cout, a, None) == -1
        assert L.lidar_wino43s_conv3x3_nhwc(a, 1, 8, 8, cin, max(cin, 4), a, None, 0, cout, a, max(cout, 4), 0, None) == -1
    for cin, cout in ((32, 128), (48, 128), (80, 384), (128, 256), (256, 256), (512, 1152)):
        assert L.lidar_wino43s_supported(cin, cout) and wino.supported43_share(cin, cout)
        assert L.lidar_wino43s_packed_floats(cin, cout) == 36 * cin * cout == L.lidar_wino43_packed_floats(cin, cout), (cin, cout)
    # the launcher's other limits are those of lidar_wino43_conv3x3_nhwc
    run = lambda **k: L.lidar_wino43s_conv3x3_nhwc(*[k.get(n, d) for n, d in (("inp", a), ("B", 1), ("H", 8), ("W", 8), ("cin", 32), ("in_c", 32),       # noqa: E731
                                                                               ("packed", a), ("bias", None), ("relu", 0), ("cout", 128), ("out", a),
                                                                               ("out_c", 128), ("off", 0), ("stream", None))])
    for bad in (dict(inp=None), dict(packed=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(in_c=16), dict(in_c=34), dict(out_c=64),
                dict(off=4), dict(off=-4), dict(out_c=130), dict(out_c=136, off=2), dict(inp=C.c_void_p(0x20004)), dict(out=C.c_void_p(0x20008)),
                dict(B=4096, H=1024, W=1024)):
        assert run(**bad) == -1, bad
