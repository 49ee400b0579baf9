"""GPU checks of the train-mode BEV backbone (csrc/bn_train.hip, bev_train.py): the fused BatchNorm2d + ReLU against float64 torch,
the Winograd convolution layer forward and input gradient against float64 autograd (F(4x4) and the F(2x2) fallback), the backbone
against the reference's own float64 train step (tests/golden/bev_train_ref.npz), PointPillar and SECOND widths against the stock
train-mode modules, PointPillarKITTI.train_loss(backbone="fused") against "stock", and sync-freedom / bitwise reproducibility."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gpu_util import no_host_sync, pp_inputs, rel, release_memory  # noqa: F401  (release_memory: an autouse fixture)
from lidardetection_amd import bev_train, wino
from lidardetection_amd.pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
from lidardetection_amd.pointpillar import make_bev_backbone

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


FIXTURE_CFG = _Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[2, 2], NUM_FILTERS=[64, 32], UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[64, 64])


# The noise floor of the comparisons with the stock modules: the stock step rerun on inputs perturbed by NOISE (relative).  The
# fused path's forward differs from the stock one by the Winograd F(4x4, 3x3) error, ~1e-5 of the output scale, not
# by fp32 rounding: near-zero pre-activations then fall on the other side of the ReLU, and each such flip moves a BatchNorm-
# normalised gradient sum by one element's share.  2^-24 noise flips almost none of them (a floor of exactly 0 for some dbeta),
# so the floor is taken at the Winograd error's size.
NOISE = 2.0 ** -17


def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(DEV)


def _bn(c, seed):
    bn = nn.BatchNorm2d(c, eps=1e-3, momentum=0.01).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        gamma = torch.empty(c).uniform_(0.5, 1.5, generator=g)
        gamma[::3] *= -1.0                                           # negative gammas
        bn.weight.copy_(gamma)
        bn.bias.copy_(torch.empty(c).uniform_(-0.5, 0.5, generator=g))
        bn.running_mean.copy_(torch.empty(c).uniform_(-0.2, 0.2, generator=g))
        bn.running_var.copy_(torch.empty(c).uniform_(0.7, 1.3, generator=g))
    return bn.train()


def _ref_bn_relu(zs, bns):
    """float64 F.batch_norm(training=True) + ReLU of each input -> (y cat, [(mean, biased var)])"""
    ys, st = [], []
    for z, bn in zip(zs, bns):
        z64 = z.double()
        ys.append(torch.relu(F.batch_norm(z64, None, None, bn.weight.double(), bn.bias.double(), True, 0.0, bn.eps)))
        st.append((z64.mean(dim=(0, 2, 3)), z64.var(dim=(0, 2, 3), unbiased=False)))
    return torch.cat(ys, 1), st


@pytest.mark.parametrize("shapes", [[(2, 64, 7, 9)], [(3, 128, 5, 11)], [(2, 256, 3, 5)], [(16, 64, 248, 216)],
                                    [(2, 128, 9, 7), (2, 128, 9, 7), (2, 128, 9, 7)]],
                         ids=["c64_odd", "c128_odd", "c256_odd", "pp_block1_bs16", "deblocks_x3"])
def test_bn_relu_kernels_match_float64(shapes):
    zs = [_randn(s, 10 + i, 1.7, 0.8).contiguous(memory_format=CL).requires_grad_() for i, s in enumerate(shapes)]
    bns = [_bn(s[1], 20 + i) for i, s in enumerate(shapes)]
    stock = [copy.deepcopy(b) for b in bns]
    y = bev_train.bn_relu_train(zs, bns)
    assert y.is_contiguous(memory_format=CL) and y.shape[1] == sum(s[1] for s in shapes)
    ref, st = _ref_bn_relu([z.detach() for z in zs], bns)
    assert rel(y, ref) < 1e-5
    G = _randn(y.shape, 7).contiguous(memory_format=CL)
    (y * G).sum().backward()
    z64 = [z.detach().double().requires_grad_() for z in zs]
    g64 = [bn.weight.detach().double().requires_grad_() for bn in bns]
    b64 = [bn.bias.detach().double().requires_grad_() for bn in bns]
    ref = torch.cat([torch.relu(F.batch_norm(z, None, None, g, b, True, 0.0, bn.eps)) for z, g, b, bn in zip(z64, g64, b64, bns)], 1)
    (ref * G.double()).sum().backward()
    for z, r in zip(zs, z64):
        assert rel(z.grad, r.grad) < 1e-5
    for bn, g, b in zip(bns, g64, b64):
        assert rel(bn.weight.grad, g.grad) < 1e-5 and rel(bn.bias.grad, b.grad) < 1e-5
    for z, bn, sb, (mu, var) in zip(zs, bns, stock, st):
        sb(z.detach())                                               # torch's own running update on the same input
        torch.testing.assert_close(bn.running_mean, sb.running_mean, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(bn.running_var, sb.running_var, rtol=1e-6, atol=1e-7)
        assert int(bn.num_batches_tracked) == int(sb.num_batches_tracked) == 1
        n = z.numel() // z.shape[1]
        _, _, _, bstats = bev_train.bn_relu_forward([z.detach()], bn.weight.detach(), bn.bias.detach(), bn.eps)
        c = z.shape[1]
        assert rel(bstats[:c], mu) < 1e-6 or float((bstats[:c].double() - mu).abs().max()) < 1e-7
        assert rel(bstats[c:2 * c], var) < 1e-6
        assert rel(bstats[2 * c:], var * n / (n - 1)) < 1e-6


def test_bn_relu_channel_slices_in_and_out():
    parent = _randn((2, 192, 9, 13), 3, 1.3, -0.4).contiguous(memory_format=CL)
    z = parent[:, 32:160]                                            # a 128-channel slice at row stride 192
    bn = _bn(128, 5)
    out = torch.full((2, 256, 9, 13), 7.0, device=DEV).contiguous(memory_format=CL)
    y, stats, ss, _ = bev_train.bn_relu_forward([z], bn.weight.detach(), bn.bias.detach(), bn.eps, out=out, out_offset=64)
    ref, _ = _ref_bn_relu([z], [bn])
    assert y is out and rel(out[:, 64:192], ref) < 1e-5
    assert bool((out[:, :64] == 7.0).all()) and bool((out[:, 192:] == 7.0).all())          # nothing outside the slice is touched
    gpar = _randn((2, 300, 9, 13), 4).contiguous(memory_format=CL)
    g = gpar[:, 100:228]                                             # the gradient read from a slice of a wider map too
    (dz,), dg, db = bev_train.bn_relu_backward([z], gpar, bn.weight.detach(), stats, ss, grad_offset=100)
    z64 = z.double().requires_grad_()
    w64, b64 = bn.weight.detach().double().requires_grad_(), bn.bias.detach().double().requires_grad_()
    (torch.relu(F.batch_norm(z64, None, None, w64, b64, True, 0.0, bn.eps)) * g.double()).sum().backward()
    assert dz.shape == z.shape and rel(dz, z64.grad) < 1e-5
    assert rel(dg, w64.grad) < 1e-5 and rel(db, b64.grad) < 1e-5


@pytest.mark.parametrize("cin,cout,hw,force_f23", [(64, 64, (30, 26), False), (128, 128, (17, 23), False), (64, 128, (20, 20), False),
                                                   (64, 64, (30, 26), True), (32, 32, (13, 15), False)])
def test_wino_conv_layer_forward_and_input_grad(monkeypatch, cin, cout, hw, force_f23):
    if force_f23:                                                    # every map "too large" for F(4x4): the F(2x2) fallback
        monkeypatch.setattr(wino, "_F43_MAX_BYTES", [1])
    x = _randn((2, cin) + hw, 31).contiguous(memory_format=CL).requires_grad_()
    w = (_randn((cout, cin, 3, 3), 32) / (9 * cin) ** 0.5).contiguous(memory_format=CL).requires_grad_()
    z = bev_train.conv3x3_train(x, w)
    G = _randn(z.shape, 33).contiguous(memory_format=CL)
    (z * G).sum().backward()
    x64, w64 = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    z64 = F.conv2d(x64, w64, None, 1, 1)
    (z64 * G.double()).sum().backward()
    assert rel(z, z64) < 1e-4
    assert rel(x.grad, x64.grad) < 1e-4
    assert rel(w.grad, w64.grad) < 1e-4


def _fixture_model(z):
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    sd = {}
    for k, v in m.state_dict().items():
        a = torch.from_numpy(z["bev." + k])
        sd[k] = a.float() * float(z["weight_scale"]) if a.dtype == torch.int8 else a
    m.load_state_dict(sd)
    return m.to(DEV).to(memory_format=CL).train()


def test_backbone_matches_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "bev_train_ref.npz"))
    m = _fixture_model(z)
    assert bev_train.TrainBEVBackbone(m.blocks, m.deblocks).routes() == ([["conv", "wino"], ["conv", "wino"]], ["fused", "fused"])
    x = (torch.from_numpy(z["x_code"]).float() * float(z["x_scale"])).to(DEV).contiguous(memory_format=CL).requires_grad_()
    G = (torch.from_numpy(z["g_code"]).float() * float(z["g_scale"])).to(DEV).contiguous(memory_format=CL)
    y = m({"spatial_features": x})["spatial_features_2d"]            # the mirror routes train-mode channels-last maps to TrainBEVBackbone
    assert rel(y, torch.from_numpy(z["out64"]).to(DEV)) < 1e-5
    (y * G).sum().backward()
    assert rel(x.grad, torch.from_numpy(z["dx64"]).to(DEV)) < 1e-4
    for name, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            assert rel(mod.weight.grad, torch.from_numpy(z["d_gamma." + name]).to(DEV)) < 1e-4, name
            assert rel(mod.bias.grad, torch.from_numpy(z["d_beta." + name]).to(DEV)) < 1e-4, name
            torch.testing.assert_close(mod.running_mean, torch.from_numpy(z["rm1." + name]).to(DEV), rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(mod.running_var, torch.from_numpy(z["rv1." + name]).to(DEV), rtol=1e-5, atol=1e-6)
            assert int(mod.num_batches_tracked) == 1
        elif isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            key = name + ".weight"
            ref = torch.from_numpy(z["dw16." + key].astype(np.float32)).to(DEV) * float(z["dw_scale." + key])
            assert rel(mod.weight.grad, ref) < 2e-3, name                 # float16 storage


def _three(make, seed):
    torch.manual_seed(seed)
    blocks, deblocks = make()
    mods = nn.ModuleList([blocks, deblocks]).to(DEV).to(memory_format=CL).train()
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    with torch.no_grad():
        for m in mods.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty(m.num_features).uniform_(-0.3, 0.3, generator=g))
    return mods, copy.deepcopy(mods), copy.deepcopy(mods)


def _stock_forward(mods, x):
    blocks, deblocks = mods
    ups = []
    for blk, de in zip(blocks, deblocks):
        x = blk(x)
        ups.append(de(x))
    return torch.cat(ups, 1)


@pytest.mark.parametrize("which", ["pointpillar", "second"])
def test_widths_match_stock_train_modules(which):
    if which == "pointpillar":
        make, shape = make_bev_backbone, (2, 64, 96, 88)
    else:
        make = lambda: make_bev_backbone(cin=256, layer_nums=(5, 5), strides=(1, 2), filters=(128, 256), up_strides=(1, 2),  # noqa: E731
                                         up_filters=(256, 256))
        shape = (2, 256, 40, 44)
    fused, stock, noisy = _three(make, 3)
    x0 = torch.relu(_randn(shape, 41)).contiguous(memory_format=CL)
    xs = [x0.clone().requires_grad_() for _ in range(3)]
    tb = bev_train.TrainBEVBackbone(fused[0], fused[1])
    assert all(r != "stock" for blk in tb.routes()[0] for r in blk)
    yf = tb(xs[0])
    ys = _stock_forward(stock, xs[1])
    noise = 1 + NOISE * _randn(shape, 42)
    yn = _stock_forward(noisy, (xs[2] * noise).contiguous(memory_format=CL))
    assert rel(yf, ys) < 1e-4
    G = _randn(yf.shape, 43).contiguous(memory_format=CL)
    for y in (yf, ys, yn):
        (y * G).sum().backward()
    floor = rel(xs[2].grad, xs[1].grad)
    assert rel(xs[0].grad, xs[1].grad) < max(1e-4, 10 * floor)
    pf, ps, pn = dict(fused.named_parameters()), dict(stock.named_parameters()), dict(noisy.named_parameters())
    bad = {}
    for k in ps:
        err, fl = rel(pf[k].grad, ps[k].grad), rel(pn[k].grad, ps[k].grad)
        if not err < max(1e-4, 10 * fl):
            bad[k] = (err, fl)
    assert not bad, bad
    for (k, bf), bs in zip(fused.named_buffers(), stock.buffers()):
        if "running" in k:
            torch.testing.assert_close(bf, bs, rtol=1e-5, atol=1e-6)
        else:
            assert int(bf) == int(bs) == 1


def test_train_loss_fused_matches_stock_and_refolds():
    from lidardetection_amd import pillar_ops
    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = pp_inputs(2, 5, 2300)
    models = []
    for _ in range(3):
        torch.manual_seed(6)
        models.append(PointPillarKITTI(batch_size=2, device=DEV))
    fused, stock, noisy = models
    canvas = torch.relu(_randn((2, 64, fused.ny, fused.nx), 8)).contiguous(memory_format=CL)
    fused.backbone_head(canvas)                                      # a folded backbone exists before the training step
    for m in models:
        m.train()
    with pytest.raises(pillar_ops._lib.LidarHipError):
        fused.train_loss(pts, offs, gt, backbone="folded")
    orig = noisy.backbone_head_stock
    noisy.backbone_head_stock = lambda c: orig(c * (1 + NOISE * _randn(c.shape, 9)))
    lf = fused.train_loss(pts, offs, gt, backbone="fused")
    ls = stock.train_loss(pts, offs, gt)
    ln = noisy.train_loss(pts, offs, gt)
    for a, b in zip(lf, ls):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    for ll in (lf, ls, ln):
        sum(ll).backward()
    pf, ps, pn = dict(fused.named_parameters()), dict(stock.named_parameters()), dict(noisy.named_parameters())
    errs = {k: rel(p.grad, ps[k].grad) for k, p in pf.items() if p.grad is not None}
    assert len(errs) == len(ps)
    bad = {k: (v, rel(pn[k].grad, ps[k].grad)) for k, v in errs.items() if not v < max(1e-4, 10 * rel(pn[k].grad, ps[k].grad))}
    assert not bad, bad
    for (k, bf), bs in zip(fused.named_buffers(), stock.buffers()):
        if "running" in k:
            torch.testing.assert_close(bf, bs, rtol=1e-5, atol=1e-6)
        elif "num_batches" in k:
            assert int(bf) == int(bs) == 1
    fused.eval()
    fresh = PointPillarKITTI(batch_size=2, device=DEV).eval()
    fresh.load_state_dict(fused.state_dict())
    with torch.no_grad():
        a, b = fused.backbone_head(canvas)[0], fresh.backbone_head(canvas)[0]
    assert torch.equal(a, b)                                         # the folded forward refolded with the new statistics


def test_sync_free_and_bitwise_deterministic():
    """the whole backbone step runs without a host synchronisation; the fused kernels' results (a chain of this package's layers
    only: Winograd forward and input gradient, fused BN + ReLU with one and with two inputs) are bitwise equal across runs.  The
    full backbone is not compared bit for bit: its stride-2 and deblock convolutions run in MIOpen, whose fp32 channels-last solvers
    may accumulate in a run-dependent order (as the weight gradients, excluded here for the same reason)."""
    torch.manual_seed(12)
    blocks, deblocks = make_bev_backbone()
    base = nn.ModuleList([blocks, deblocks]).to(DEV).to(memory_format=CL).train()
    x0 = torch.relu(_randn((2, 64, 128, 112), 13)).contiguous(memory_format=CL)
    w1 = (_randn((128, 64, 3, 3), 15) / 24.0).contiguous(memory_format=CL)
    w2 = (_randn((128, 128, 3, 3), 16) / 34.0).contiguous(memory_format=CL)
    bn_base = [_bn(128, 17), _bn(128, 18), _bn(128, 19)]
    G = _randn((2, 384, 64, 56), 14).contiguous(memory_format=CL)
    Gc = _randn((2, 256, 128, 112), 20).contiguous(memory_format=CL)
    outs = []
    for rep in range(3):                                             # rep 0 warms the libraries up outside the sync check
        mods = copy.deepcopy(base)
        bns = [copy.deepcopy(b) for b in bn_base]
        x, xc = x0.clone().requires_grad_(), x0.clone().requires_grad_()
        tb = bev_train.TrainBEVBackbone(mods[0], mods[1])
        with no_host_sync(rep > 0):
            y = tb(x)
            (y * G).sum().backward()
            z1 = bev_train.conv3x3_train(xc, w1)
            a = bev_train.bn_relu_train(z1, bns[0])
            yc = bev_train.bn_relu_train([bev_train.conv3x3_train(a, w2), z1], bns[1:])
            (yc * Gc).sum().backward()
        outs.append([yc.detach(), xc.grad] + [t for b in bns for t in (b.running_mean, b.running_var, b.weight.grad, b.bias.grad)])
        assert y.shape == G.shape and x.grad is not None
    for a, b in zip(outs[1], outs[2]):
        assert torch.equal(a, b)
