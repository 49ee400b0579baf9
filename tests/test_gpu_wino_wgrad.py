"""GPU checks of the Winograd F(3x3, 4x4) weight-gradient kernel (csrc/wino43_wgrad.hip, wino.conv3x3_wgrad_f43) and of the
wgrad="wino" option of bev_train / pointpillar: the kernel against float64 (small, odd and production shapes, channel slices),
bitwise reproducibility and independence of the workspace's contents, autograd, the backbone against the reference's own train
step (tests/golden/bev_train_ref.npz), PointPillar widths and the whole training step against the "library" option, sync-freedom.

Measured on an MI355X, max |dW - float64| / max |float64| (test_production_shapes_match_float64, printed by the test):
    (16, 64, 248, 216): kernel 5.6e-6, library 1.2e-6;  (16, 128, 124, 108): 6.2e-6 / 7.5e-7;  (16, 256, 62, 54): 8.5e-6 / 8.8e-7;
the small shapes of test_kernel_matches_float64: 3.1e-7 .. 2.3e-6.  The bar is 1e-4."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from _gpu_util import no_host_sync, pp_inputs, rel, release
from lidardetection_amd import bev_train, wino, workspace
from lidardetection_amd.pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
from lidardetection_amd.pointpillar import make_bev_backbone

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last
BAR = 1e-4                 # the tolerance the project states once for all fp32 results (README "Parity")
NOISE = 2.0 ** -17         # the noise floor of tests/test_gpu_bev_train.py: the Winograd forward's error size


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


FIXTURE_CFG = _Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[2, 2], NUM_FILTERS=[64, 32], UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[64, 64])


@pytest.fixture(autouse=True, scope="module")
def _release_memory():
    yield
    release("wino43_wgrad")


def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(DEV)


def _map(shape, seed, relu):
    """(B, C, H, W) channels-last map with canonical strides; relu: a post-ReLU activation (zeros and a non-zero mean)"""
    B, C, H, W = shape
    t = _randn((B, H, W, C), seed, 1.0, 0.3 if relu else 0.0)
    return (torch.relu(t) if relu else t).permute(0, 3, 1, 2)


def _ref64(x, g):
    B, cin, H, W = x.shape
    w = torch.zeros((g.shape[1], cin, 3, 3), dtype=torch.float64, device=x.device)
    return torch.ops.aten.convolution_backward(g.double(), x.double(), w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


SMALL = [(2, 64, 30, 26), (2, 128, 17, 23), (3, 256, 7, 9), (1, 64, 3, 2), (2, 64, 4, 4), (2, 128, 5, 1), (1, 512, 6, 5)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "slices"])
def test_kernel_matches_float64(shape, sliced):
    B, C, H, W = shape
    if sliced:                                                       # x and g as channel slices of wider maps
        x = _map((B, C + 96, H, W), 1, True)[:, 32:32 + C]
        g = _map((B, C + 40, H, W), 2, False)[:, 8:8 + C]
        assert x.stride(3) == C + 96 and g.stride(3) == C + 40
    else:
        x, g = _map(shape, 1, True), _map(shape, 2, False)
    dw = wino.conv3x3_wgrad_f43(x, g)
    assert dw.shape == (C, C, 3, 3) and dw.is_contiguous() and dw.dtype == torch.float32
    err = rel(dw, _ref64(x, g))
    print(f"wgrad43 {shape} sliced={sliced}: {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("shape", [(16, 64, 248, 216), (16, 128, 124, 108), (16, 256, 62, 54)], ids=lambda s: "x".join(map(str, s)))
def test_production_shapes_match_float64(shape):
    x, g = _map(shape, 3, True), _map(shape, 4, False)
    ref = _ref64(x, g)
    dw = wino.conv3x3_wgrad_f43(x, g)
    w = torch.zeros((shape[1], shape[1], 3, 3), device=DEV).contiguous(memory_format=CL)
    lib = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    err, err_lib = rel(dw, ref), rel(lib, ref)
    print(f"wgrad43 {shape}: kernel {err:.3e}  library {err_lib:.3e}")
    assert err <= BAR


def test_reproducible_and_workspace_independent():
    shape = (2, 64, 30, 26)
    x, g = _map(shape, 5, True), _map(shape, 6, False)
    a = wino.conv3x3_wgrad_f43(x, g)
    b = wino.conv3x3_wgrad_f43(x, g)
    assert torch.equal(a, b)
    wsb = wino._lib.lib().lidar_wino43_wgrad_workspace_bytes(*[shape[i] for i in (0, 2, 3)], 64, 64)
    ws = workspace.get("wino43_wgrad", wsb, DEV)
    ws.view(torch.float32).fill_(float("nan"))
    c = wino.conv3x3_wgrad_f43(x, g)
    assert workspace.get("wino43_wgrad", wsb, DEV) is ws             # the call above used the poisoned buffer
    assert torch.equal(a, c)
    # dW pre-filled with NaN comes back finite: overwritten, not accumulated into (the raw entry point, on a buffer of ours)
    dw = torch.full((64, 64, 3, 3), float("nan"), device=DEV)
    L, lib = wino._lib.lib(), wino._lib
    lib.check(L.lidar_wino43_wgrad_nhwc(lib.ptr(x), 64, lib.ptr(g), 64, 2, 30, 26, 64, 64, lib.ptr(dw), lib.ptr(ws), wsb, lib.stream()), "wgrad")
    assert bool(torch.isfinite(dw).all()) and torch.equal(dw, a)


def test_host_errors_on_device_tensors():
    x, g = _map((2, 64, 8, 8), 7, True), _map((2, 64, 8, 8), 8, False)
    E = wino._lib.LidarHipError
    with pytest.raises(E):
        wino.conv3x3_wgrad_f43(x, g[:, :48])                         # unsupported width
    with pytest.raises(E):
        wino.conv3x3_wgrad_f43(x, g[:, :, :4])                       # shapes differ
    with pytest.raises(E):
        wino.conv3x3_wgrad_f43(x.contiguous(), g)                    # not channels-last
    with pytest.raises(E):
        wino.conv3x3_wgrad_f43(x.double(), g)
    with pytest.raises(E):
        wino.conv3x3_wgrad_f43(x.cpu(), g)


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, (30, 26)), (128, 128, (17, 23)), (64, 128, (20, 20))])
def test_autograd(cin, cout, hw):
    x0 = torch.relu(_randn((2, cin) + hw, 31, 1.0, 0.3)).contiguous(memory_format=CL)
    w0 = (_randn((cout, cin, 3, 3), 32) / (9 * cin) ** 0.5).contiguous(memory_format=CL)
    res = {}
    for opt in ("wino", "library"):
        x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
        z = bev_train.conv3x3_train(x, w, wgrad=opt)
        G = _randn(z.shape, 33).contiguous(memory_format=CL)
        (z * G).sum().backward()
        res[opt] = (z.detach(), x.grad.clone(), w.grad.clone(), x, w, G)
    x64, w64 = x0.double().requires_grad_(), w0.double().requires_grad_()
    (torch.nn.functional.conv2d(x64, w64, None, 1, 1) * res["wino"][5].double()).sum().backward()
    assert torch.equal(res["wino"][0], res["library"][0])            # the forward is untouched
    assert torch.equal(res["wino"][1], res["library"][1])            # ... and so is the input gradient
    assert rel(res["wino"][2], w64.grad) <= BAR
    # accumulation: a second backward into the same .grad gives twice the single one, to fp32 rounding
    _, _, single, x, w, G = res["wino"]
    (bev_train.conv3x3_train(x, w, wgrad="wino") * G).sum().backward()
    assert rel(w.grad, 2 * single) <= 2.0 ** -22


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
    x0 = (torch.from_numpy(z["x_code"]).float() * float(z["x_scale"])).to(DEV).contiguous(memory_format=CL)
    G = (torch.from_numpy(z["g_code"]).float() * float(z["g_scale"])).to(DEV).contiguous(memory_format=CL)
    ys = []
    for opt in ("library", "library", "wino"):
        m = _fixture_model(z)
        tb = bev_train.TrainBEVBackbone(m.blocks, m.deblocks, wgrad=opt)
        x = x0.clone().requires_grad_()
        ys.append(tb(x))
    assert tb.routes() == ([["conv", "wino"], ["conv", "wino"]], ["fused", "fused"])
    assert tb.wgrad_routes() == [[None, "wino"], [None, "wino"]]     # 64 -> 64 and 32 -> 32: both widths are supported
    y = ys[2]
    assert rel(y, torch.from_numpy(z["out64"]).to(DEV)) < 1e-5
    if torch.equal(ys[0], ys[1]):                                    # the library-option forward is bitwise stable here: ours equals it
        assert torch.equal(y, ys[0])
    (y * G).sum().backward()
    assert rel(x.grad, torch.from_numpy(z["dx64"]).to(DEV)) < 1e-4
    for name, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            assert rel(mod.weight.grad, torch.from_numpy(z["d_gamma." + name]).to(DEV)) < 1e-4, name
            assert rel(mod.bias.grad, torch.from_numpy(z["d_beta." + name]).to(DEV)) < 1e-4, name
        elif isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            key = name + ".weight"
            ref = torch.from_numpy(z["dw16." + key].astype(np.float32)).to(DEV) * float(z["dw_scale." + key])
            assert rel(mod.weight.grad, ref) < 2e-3, name           # float16 storage


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


def test_pointpillar_widths_match_library_option():
    """the "wino" backbone against the "library" one, with the noise floor of tests/test_gpu_bev_train.py: the library backbone
    rerun on an input perturbed by NOISE (the MIOpen layers that remain move the last bits run to run)"""
    shape = (2, 64, 96, 88)
    new, lib, noisy = _three(make_bev_backbone, 3)
    x0 = torch.relu(_randn(shape, 41)).contiguous(memory_format=CL)
    xs = [x0.clone().requires_grad_() for _ in range(3)]
    tb = bev_train.TrainBEVBackbone(new[0], new[1], wgrad="wino")
    routes = tb.wgrad_routes()
    assert [r for blk in routes for r in blk].count("wino") == 13 and "library" not in [r for blk in routes for r in blk]
    assert tb.routes() == bev_train.TrainBEVBackbone(lib[0], lib[1]).routes()
    yw = tb(xs[0])
    yl = bev_train.TrainBEVBackbone(lib[0], lib[1])(xs[1])
    noise = 1 + NOISE * _randn(shape, 42)
    yn = bev_train.TrainBEVBackbone(noisy[0], noisy[1])((xs[2] * noise).contiguous(memory_format=CL))
    assert rel(yw, yl) < 1e-4
    G = _randn(yw.shape, 43).contiguous(memory_format=CL)
    for y in (yw, yl, yn):
        (y * G).sum().backward()
    assert rel(xs[0].grad, xs[1].grad) < max(1e-4, 10 * rel(xs[2].grad, xs[1].grad))
    pw, pl, pn = dict(new.named_parameters()), dict(lib.named_parameters()), dict(noisy.named_parameters())
    bad = {}
    for k in pl:
        assert pw[k].grad is not None and bool(torch.isfinite(pw[k].grad).all()), k
        err, fl = rel(pw[k].grad, pl[k].grad), rel(pn[k].grad, pl[k].grad)
        if not err < max(1e-4, 10 * fl):
            bad[k] = (err, fl)
    assert not bad, bad


def test_train_loss_wino_matches_library_option():
    from lidardetection_amd import pillar_ops
    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = pp_inputs(2, 5, 2300)
    models = []
    for _ in range(3):
        torch.manual_seed(6)
        models.append(PointPillarKITTI(batch_size=2, device=DEV).train())
    new, lib, noisy = models
    with pytest.raises(pillar_ops._lib.LidarHipError):
        new.train_loss(pts, offs, gt, backbone="fused", wgrad="nonsense")
    orig = noisy.backbone_head_train
    noisy.backbone_head_train = lambda c, wgrad="library": orig((c * (1 + NOISE * _randn(c.shape, 9))).contiguous(memory_format=CL), wgrad)
    lw = new.train_loss(pts, offs, gt, backbone="fused", wgrad="wino")
    ll = lib.train_loss(pts, offs, gt, backbone="fused")
    ln = noisy.train_loss(pts, offs, gt, backbone="fused")
    for a, b in zip(lw, ll):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    for losses in (lw, ll, ln):
        sum(losses).backward()
    pw, pl, pn = dict(new.named_parameters()), dict(lib.named_parameters()), dict(noisy.named_parameters())
    errs = {k: rel(p.grad, pl[k].grad) for k, p in pw.items() if p.grad is not None and bool(torch.isfinite(p.grad).all())}
    assert len(errs) == len(pl)                                      # every parameter received a finite gradient
    bad = {k: (v, rel(pn[k].grad, pl[k].grad)) for k, v in errs.items() if not v < max(1e-4, 10 * rel(pn[k].grad, pl[k].grad))}
    assert not bad, bad
    routes = [r for blk in new.__dict__["_bev_train_wino"].wgrad_routes() for r in blk]
    assert routes.count("wino") == 13 and "library" not in routes


def test_sync_free():
    torch.manual_seed(12)
    blocks, deblocks = make_bev_backbone()
    base = nn.ModuleList([blocks, deblocks]).to(DEV).to(memory_format=CL).train()
    x0 = torch.relu(_randn((2, 64, 128, 112), 13)).contiguous(memory_format=CL)
    G = _randn((2, 384, 64, 56), 14).contiguous(memory_format=CL)
    grads = []
    for rep in range(3):                                             # rep 0 warms the libraries and the workspace up outside the check
        mods = copy.deepcopy(base)
        x = x0.clone().requires_grad_()
        tb = bev_train.TrainBEVBackbone(mods[0], mods[1], wgrad="wino")
        with no_host_sync(rep > 0):
            (tb(x) * G).sum().backward()
        assert x.grad is not None
        grads.append(mods)
    for p in grads[2].parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
