"""CPU checks of what the dense BEV paths share: the block parser and its records (bev_backbone.parse_block / BlockLayer, read by
FoldedBEVBackbone and by bev_train), the folded stage records a FoldedBEVBackbone keeps, the agreement of the inference and the
train routing on which layers are Winograd layers, and the F(4x4) / F(2x2) rule (wino.kernel_for).  Nothing is launched."""
import pytest
import torch.nn as nn

from lidardetection_amd import bev_backbone as bb
from lidardetection_amd import bev_train, wino
from lidardetection_amd.pointpillar import make_bev_backbone

# the three settings of tests/test_gpu_pointpillar_path.py::test_folded_bev_backbone_conv_settings_vs_fp64_stock:
# case -> (ZeroPad2d, second conv's padding, dilation, groups)
ODD = {"asymmetric_zero_pad": ((0, 1, 0, 1), 1, 1, 1), "dilation": (1, 2, 2, 1), "groups": (1, 1, 1, 2)}


def _odd_block(case):
    zp, pad, dil, groups = ODD[case]
    return nn.Sequential(
        nn.ZeroPad2d(zp), nn.Conv2d(64, 64, 3, stride=2, padding=0, bias=False), nn.BatchNorm2d(64, eps=1e-3), nn.ReLU(),
        nn.Conv2d(64, 64, 3, padding=pad, dilation=dil, groups=groups, bias=False), nn.BatchNorm2d(64, eps=1e-3), nn.ReLU())


def _fields(l):
    return tuple(l.conv.stride), l.pad, l.zero_pad, l.plain3x3


def test_parser_records_of_the_pointpillar_backbone():
    blocks, _ = make_bev_backbone()
    for blk, n in zip(blocks, (3, 5, 5)):
        layers = bb.parse_block(blk)
        assert len(layers) == 1 + n
        assert _fields(layers[0]) == ((2, 2), (1, 1), None, False)         # ZeroPad2d(1) folded into the stride-2 conv's padding 0
        assert isinstance(layers[0].zpad, nn.ZeroPad2d) and layers[0].conv is blk[1] and layers[0].bn is blk[2] and layers[0].act is blk[3]
        for l in layers[1:]:
            assert _fields(l) == ((1, 1), (1, 1), None, True) and l.zpad is None


@pytest.mark.parametrize("case", sorted(ODD))
def test_parser_records_of_the_odd_conv_settings(case):
    first, second = bb.parse_block(_odd_block(case))
    want_first = {"asymmetric_zero_pad": ((2, 2), (0, 0), (0, 1, 0, 1), False)}.get(case, ((2, 2), (1, 1), None, False))
    assert _fields(first) == want_first
    assert _fields(second) == {"asymmetric_zero_pad": ((1, 1), (1, 1), None, True), "dilation": ((1, 1), (2, 2), None, False),
                               "groups": ((1, 1), (1, 1), None, False)}[case]


def test_parser_refuses_other_structures_and_keeps_what_cannot_be_folded():
    conv, bn = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
    assert bb.parse_block(nn.Sequential(conv, bn)) is None                                   # no ReLU
    assert bb.parse_block(nn.Sequential(conv, bn, nn.ReLU(), conv, bn)) is None
    assert bb.parse_block(nn.Sequential(conv, bn, nn.ReLU(), nn.ZeroPad2d(1))) is None       # dangling ZeroPad2d
    assert bb.parse_block(nn.Sequential(conv, nn.ReLU(), bn)) is None
    assert bb.parse_block(nn.Sequential()) == []
    # no explicit zero padding to fold into: pad is None, the ZeroPad2d stays aside, never a Winograd layer
    for odd in (nn.Conv2d(64, 64, 3, padding="same", bias=False), nn.Conv2d(64, 64, 3, padding=1, padding_mode="reflect", bias=False)):
        (l,) = bb.parse_block(nn.Sequential(nn.ZeroPad2d(1), odd, bn, nn.ReLU()))
        assert l.pad is None and l.zero_pad == (1, 1, 1, 1) and not l.plain3x3
        assert bev_train.conv_route(odd, bn, (1, 1, 1, 1)) == "stock"
    (l,) = bb.parse_block(nn.Sequential(nn.ZeroPad2d(-1), nn.Conv2d(64, 64, 3, padding=2, bias=False), bn, nn.ReLU()))
    assert l.pad == (2, 2) and l.zero_pad == (-1, -1, -1, -1) and not l.plain3x3            # a crop is not padding


@pytest.mark.parametrize("case", sorted(ODD))
def test_folded_backbone_records_on_cpu_modules(case):
    """the (zero_pad, pad, dilation, groups) values test_folded_bev_backbone_conv_settings_vs_fp64_stock asserts on the GPU, from CPU
    modules: building the records calls nothing in the library (no Winograd filters, no packed deblock weight, no sparse first layer)"""
    blocks = nn.ModuleList([_odd_block(case)]).eval()
    deblocks = nn.ModuleList([nn.Sequential(nn.ConvTranspose2d(64, 128, 2, stride=2, bias=False), nn.BatchNorm2d(128, eps=1e-3),
                                            nn.ReLU())]).eval()
    bev = bb.FoldedBEVBackbone(blocks, deblocks, [nn.Conv2d(128, 18, 1)])
    (convs, up), = bev.stages
    assert (convs[0].zero_pad, convs[0].pad, convs[1].pad, convs[1].dilation, convs[1].groups) == \
        {"asymmetric_zero_pad": ((0, 1, 0, 1), (0, 0), (1, 1), (1, 1), 1), "dilation": (None, (1, 1), (2, 2), (2, 2), 1),
         "groups": (None, (1, 1), (1, 1), (1, 1), 2)}[case]
    assert convs[0].stride == (2, 2) and convs[1].stride == (1, 1) and all(cv.wino is None for cv in convs)
    assert (up.kind, up.packed, up.stride, up.args) == ("gemm", None, 2, ()) and tuple(up.weight.shape) == (64, 2 * 2 * 128)
    assert bev.up_channels == [128] and bev.head_split == [18] and not bev.sparse_first_ok()
    with pytest.raises(AssertionError):                                      # unknown block structure is still refused
        bb.FoldedBEVBackbone(nn.ModuleList([nn.Sequential(nn.Conv2d(64, 64, 3, padding=1), nn.ReLU())]), deblocks, [])


def test_library_deblock_records_keep_the_call_arguments():
    blocks, _ = make_bev_backbone(layer_nums=(1,), strides=(2,), filters=(64,), up_strides=(1,), up_filters=(64,))
    for de, want in ((nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False), ("deconv", ((2, 2), (1, 1), (1, 1)))),
                     (nn.Conv2d(64, 32, 2, stride=2, bias=False), ("conv", ((2, 2), (0, 0))))):
        deblocks = nn.ModuleList([nn.Sequential(de, nn.BatchNorm2d(32), nn.ReLU())])
        (_, up), = bb.FoldedBEVBackbone(blocks.eval(), deblocks.eval(), []).stages
        assert (up.kind, up.args, up.stride, up.packed) == (*want, 0, None) and up.shift.numel() == 32


def test_train_and_inference_agree_on_the_winograd_layers():
    """conv_route says "wino" exactly for the layers whose record is a plain 3x3 and whose widths the train kernels take; the
    inference side packs Winograd filters under the same property with wino.supported"""
    blocks = list(make_bev_backbone()[0]) + [_odd_block(c) for c in sorted(ODD)]
    blocks += list(make_bev_backbone(cin=64, layer_nums=(1, 1), strides=(1, 2), filters=(16, 40), up_strides=(1, 2), up_filters=(64, 64))[0])
    seen = set()
    for blk in blocks:
        for l in bb.parse_block(blk):
            zp = (0, 0, 0, 0) if l.zpad is None else l.zpad.padding
            cin, cout = l.conv.in_channels, l.conv.out_channels
            want = l.plain3x3 and bev_train.wino_train_supported(cin, cout)
            assert (bev_train.conv_route(l.conv, l.bn, zp) == "wino") == want, (cin, cout, _fields(l))
            assert not want or wino.supported(cin, cout)                    # a train Winograd layer is an inference Winograd layer
            seen.add((l.plain3x3, want))
        assert [r == "wino" for r in bev_train.TrainBEVBackbone([blk], []).routes()[0][0]] == \
            [l.plain3x3 and bev_train.wino_train_supported(l.conv.in_channels, l.conv.out_channels) for l in bb.parse_block(blk)]
    assert seen == {(True, True), (True, False), (False, False)}            # plain and taken, plain but too narrow, not plain


def test_winograd_kernel_rule(monkeypatch):
    small = (2, 64, 12, 10)
    assert wino.supported43(64, 64) and wino.kernel_for(64, 64, small) == "f43" and wino.kernel_for(64, 64) == "f43"
    assert wino.supported(64, 32) and not wino.supported43(64, 32)          # a width only F(2x2) takes
    assert wino.kernel_for(64, 32, small) == "f23" and wino.kernel_for(64, 32) == "f23"
    for cin, cout in ((32, 64), (16, 64), (48, 128), (64, 96), (256, 256)):
        assert wino.kernel_for(cin, cout, (2, cin, 12, 10)) == ("f43" if wino.supported43(cin, cout) else "f23"), (cin, cout)
    monkeypatch.setattr(wino, "_F43_MAX_BYTES", [1])                        # no map fits: F(2x2); the widths alone still say F(4x4)
    assert wino.kernel_for(64, 64, small) == "f23" and wino.kernel_for(64, 64) == "f43"
    monkeypatch.setattr(wino, "_F43_MAX_BYTES", [2 ** 31 - 1])
    monkeypatch.setattr(wino, "_F43", [False])
    assert wino.kernel_for(64, 64, small) == "f23" and wino.kernel_for(64, 64) == "f23"
