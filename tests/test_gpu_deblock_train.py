"""GPU checks of the deblock gradient kernels (csrc/deconv_train.hip: lidar_deconv_dgrad_nhwc, lidar_deconv_wgrad_nhwc) and of the
deblock="gemm" option of bev_train / pointpillar: both kernels through the raw C ABI against float64 autograd over their declared
range (channel slices of wider buffers, NaN-filled gaps and guard rows), the weight gradient's split into partials, bitwise
reproducibility and independence of the workspace's contents, deconv_train against float64 autograd and the stock module, the
backbone against the reference's own train step (tests/golden/deblock_train_ref.npz) and the whole training step against the
"library" option, sync-freedom.  The bar is the project's: err <= 1e-4 * max(1, |want|.max())."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gpu_util import no_host_sync, pp_inputs, rel, release
from lidardetection_amd import _lib, bev_train, workspace
from lidardetection_amd.pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
from lidardetection_amd.pointpillar import make_bev_backbone

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last
BAR = 1e-4                 # the tolerance the project states once for all fp32 results (README "Parity")
NOISE = 2.0 ** -17         # the noise floor of tests/test_gpu_bev_train.py
NAN = float("nan")


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


FIXTURE_CFG = _Cfg(LAYER_NUMS=[0, 0, 0], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=[16, 24, 24], UPSAMPLE_STRIDES=[1, 2, 4],
                   NUM_UPSAMPLE_FILTERS=[128, 128, 128])


@pytest.fixture(autouse=True, scope="module")
def _release_memory():
    yield
    release("deconv_wgrad")


def _within_bar(got, want):
    """-> (ok, err): err = max |got - want|, ok: err <= 1e-4 * max(1, max |want|)"""
    want = want.detach().double()
    err = float((got.detach().double() - want).abs().max())
    return err <= BAR * max(1.0, float(want.abs().max())), err


def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(DEV)


def _divup(a, b):
    return -(-a // b)


def wgrad_splits(B, h, w, K, s, c_up):
    """-> (partials, pixels per partial) of lidar_deconv_wgrad_nhwc: csrc/deconv_train.hip:247-266 (dw_plan) with DW_PIX 32 (:36),
    DW_ROWS 64 (:37), DW_COLS 128 (:38), DW_MAX_SPLIT_PIX 4096 (:41), DW_TARGET_WGS 512 (:42)"""
    P = B * h * w
    tiles = _divup(K, 64) * _divup(s * s * c_up // 32, 4)
    splits = min(max(_divup(512, tiles), _divup(P, 4096)), _divup(P, 32))
    pps = _divup(_divup(P, splits), 32) * 32
    return _divup(P, pps), pps


def _oracle(x, wt, G, s):
    """float64 F.conv_transpose2d under autograd on the device -> (y, dx, dw)"""
    x64, w64 = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv_transpose2d(x64, w64, None, s)
    (y * G.double()).sum().backward()
    return y.detach(), x64.grad, w64.grad


def _case_data(B, h, w, K, s, c_up, seed):
    x = torch.relu(_randn((B, K, h, w), seed, 1.0, 0.3))                       # a post-ReLU activation
    wt = _randn((K, c_up, s, s), seed + 1) / K ** 0.5
    G = _randn((B, c_up, s * h, s * w), seed + 2)
    return x, wt, G


M1, M2, M3, M4 = (1, 1, 1), (2, 3, 5), (2, 7, 9), (3, 11, 13)          # P = 1, 30, 126, 429: off every tile size, h != w, several frames
SWEEP = [(s, K, c_up, m) for s in (1, 2, 4) for K, c_up, m in
         [(16, 32, M4), (24, 96, M3), (64, 128, M2), (256, 256, M1), (256, 128, M3), (64, 256, M4), (24, 32, M1), (16, 128, M3),
          (256, 96, M2), (64, 32, M3)]]


def _sliced(rows, width, ld, off, data=None):
    """a (rows + 1, ld) NaN-filled buffer (one guard row) whose columns [off, off + width) of the first `rows` rows hold `data`"""
    buf = torch.full((rows + 1, ld), NAN, device=DEV)
    if data is not None:
        buf[:rows, off:off + width] = data
    return buf


def _untouched(buf, rows, width, off):
    """the gap columns and the guard row of a _sliced buffer still hold NaN"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, off:off + width] = False
    return bool(torch.isnan(buf[mask]).all())


@pytest.mark.parametrize("s,K,c_up,m", SWEEP, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_raw_kernels_match_float64(s, K, c_up, m):
    B, h, w = m
    P, Pg = B * h * w, B * h * w * s * s
    x, wt, G = _case_data(B, h, w, K, s, c_up, 100 + s + K + c_up)
    _, dx64, dw64 = _oracle(x, wt, G, s)
    x_ld, x_off, g_ld, g_off, dx_ld, dx_off = K + 8, 4, c_up + 12, 8, K + 5, 3
    xb = _sliced(P, K, x_ld, x_off, x.permute(0, 2, 3, 1).reshape(P, K))
    gb = _sliced(Pg, c_up, g_ld, g_off, G.permute(0, 2, 3, 1).reshape(Pg, c_up))
    dxb = _sliced(P, K, dx_ld, dx_off)
    dw = torch.full((K, c_up, s, s), NAN, device=DEV)
    wc = wt.contiguous()
    L = _lib.lib()
    vp = _lib.C.c_void_p
    xp, gp, dxp = vp(xb.data_ptr() + 4 * x_off), vp(gb.data_ptr() + 4 * g_off), vp(dxb.data_ptr() + 4 * dx_off)
    _lib.check(L.lidar_deconv_dgrad_nhwc(gp, g_ld, _lib.ptr(wc), B, h, w, K, s, c_up, dxp, dx_ld, _lib.stream()), "dgrad")
    wsb = L.lidar_deconv_wgrad_workspace_bytes(B, h, w, K, s, c_up)
    assert wsb == wgrad_splits(B, h, w, K, s, c_up)[0] * K * s * s * c_up * 4
    ws = torch.full((wsb // 4,), NAN, device=DEV)
    _lib.check(L.lidar_deconv_wgrad_nhwc(xp, x_ld, gp, g_ld, B, h, w, K, s, c_up, _lib.ptr(dw), _lib.ptr(ws), wsb, _lib.stream()), "wgrad")
    torch.cuda.synchronize()
    assert _untouched(dxb, P, K, dx_off)                                # gap columns and the guard row after the last pixel
    dx = dxb[:P, dx_off:dx_off + K].reshape(B, h, w, K).permute(0, 3, 1, 2)
    ok_dx, err_dx = _within_bar(dx, dx64)
    ok_dw, err_dw = _within_bar(dw, dw64)
    print(f"deblock s={s} K={K} C_up={c_up} map={m}: dgrad {err_dx:.3e} wgrad {err_dw:.3e}")
    assert bool(torch.isfinite(dw).all())                               # overwritten, never read
    assert ok_dx and ok_dw, (err_dx, err_dw)
    assert bool(torch.isfinite(ws).all())                               # every float of the workspace was written


def test_wgrad_partials():
    """the cases above cover one partial, several partials and a ragged last one (the host restatement is checked against the
    library's workspace query in every case of the sweep)"""
    assert wgrad_splits(1, 1, 1, 16, 1, 32) == (1, 32) and wgrad_splits(2, 3, 5, 64, 2, 128) == (1, 32)      # exactly one partial
    n, pps = wgrad_splits(3, 11, 13, 16, 1, 32)                          # 429 pixels, one tile: 14 partials of 32, the last holds 13
    assert (n, pps) == (14, 32) and 429 - (n - 1) * pps == 13
    n, pps = wgrad_splits(2, 7, 9, 256, 4, 128)                          # 126 pixels, 64 tiles: 4 partials of 32, the last holds 30
    assert (n, pps) == (4, 32) and 126 - 3 * 32 == 30
    n, pps = wgrad_splits(16, 248, 216, 64, 1, 128)                      # the stride-1 deblock at bs 16: 857 k pixels, one tile
    assert (n, pps) == (506, 1696) and (n - 1) * pps < 16 * 248 * 216 <= n * pps
    L = _lib.lib()
    for shape in [(16, 248, 216, 64, 1, 128), (16, 124, 108, 128, 2, 128), (16, 62, 54, 256, 4, 128), (2, 200, 176, 256, 2, 256)]:
        B, h, w, K, s, c_up = shape
        assert L.lidar_deconv_wgrad_workspace_bytes(*shape) == wgrad_splits(*shape)[0] * K * s * s * c_up * 4, shape


@pytest.mark.parametrize("s,K,c_up,m", [(1, 16, 32, M4), (2, 64, 128, M3), (4, 256, 128, M3)], ids=str)
def test_reproducible_and_workspace_independent(s, K, c_up, m):
    B, h, w = m
    x, wt, G = _case_data(B, h, w, K, s, c_up, 7)
    x, G = x.contiguous(memory_format=CL), G.contiguous(memory_format=CL)
    dx_a, dx_b = bev_train.deconv_dgrad(G, wt, s), bev_train.deconv_dgrad(G, wt, s)
    assert torch.equal(dx_a, dx_b)
    dw_a, dw_b = bev_train.deconv_wgrad(x, G, s), bev_train.deconv_wgrad(x, G, s)
    assert torch.equal(dw_a, dw_b)
    wsb = _lib.lib().lidar_deconv_wgrad_workspace_bytes(B, h, w, K, s, c_up)
    ws = workspace.get("deconv_wgrad", wsb, DEV)
    ws.view(torch.float32).fill_(NAN)
    dw_c = bev_train.deconv_wgrad(x, G, s)
    assert workspace.get("deconv_wgrad", wsb, DEV) is ws                # the call above used the poisoned buffer
    assert torch.equal(dw_a, dw_c) and torch.equal(dx_a, bev_train.deconv_dgrad(G, wt, s))


def _up(K, c_up, s, seed):
    torch.manual_seed(seed)
    up = nn.ConvTranspose2d(K, c_up, s, stride=s, bias=False)
    return up.to(DEV).to(memory_format=CL)


@pytest.mark.parametrize("K,c_up,s", [(64, 128, 1), (128, 128, 2), (256, 128, 4), (256, 256, 2)], ids=str)
def test_deconv_train_matches_float64_and_stock_module(K, c_up, s, monkeypatch):
    B, h, w = 2, 10, 7
    x0 = torch.relu(_randn((B, K, h, w), 21, 1.0, 0.3)).contiguous(memory_format=CL)
    G = _randn((B, c_up, s * h, s * w), 22).contiguous(memory_format=CL)
    up = _up(K, c_up, s, 23)
    y64, dx64, dw64 = _oracle(x0, up.weight.detach(), G, s)
    calls = _Calls(monkeypatch, (bev_train, "deconv_forward_gemm"), (bev_train, "deconv_dgrad"), (bev_train, "deconv_wgrad"))

    def run(fn):
        x, wt = x0.clone().requires_grad_(), up.weight.detach().clone().requires_grad_()
        y = fn(x, wt)
        (y * G).sum().backward()
        return y.detach(), x.grad, wt.grad

    y, dx, dw = run(lambda x, wt: bev_train.deconv_train(x, wt, s, deblock="gemm"))
    route = bev_train.deblock_conv_route(nn.Sequential(up, nn.BatchNorm2d(c_up), nn.ReLU()), "gemm")
    assert route == (("library" if (K, c_up, s) == (64, 128, 1) else "gemm"), "gemm", "gemm")
    assert calls.take() == {"deconv_forward_gemm": int(route[0] == "gemm"), "deconv_dgrad": 1, "deconv_wgrad": 1}
    assert y.is_contiguous(memory_format=CL) and dx.shape == x0.shape and dw.shape == up.weight.shape
    for name, got, want in (("y", y, y64), ("dx", dx, dx64), ("dw", dw, dw64)):
        ok, err = _within_bar(got, want)
        print(f"deconv_train ({K}, {c_up}, {s}) {name}: {err:.3e}")
        assert ok, (name, err)
    # deblock="library": torch's own call and backward, none of the kernels; bit for bit the stock module's results, compared wherever
    # the stock module, run before and after it, repeats itself bit for bit (the library may change its solver between calls)
    def stock():
        return run(lambda x, wt: F.conv_transpose2d(x, wt, None, (s, s)).contiguous(memory_format=CL))

    stock()                                                             # the library's warm-up
    before = stock()
    lib = run(lambda x, wt: bev_train.deconv_train(x, wt, s))
    after = stock()
    assert calls.take() == {"deconv_forward_gemm": 0, "deconv_dgrad": 0, "deconv_wgrad": 0}
    same = [torch.equal(before[i], after[i]) for i in range(3)]
    print(f"deconv_train ({K}, {c_up}, {s}) library: the stock module repeats itself (y, dx, dw) = {same}")
    for i in range(3):
        if same[i]:
            assert torch.equal(lib[i], before[i]), i


def test_deconv_train_weight_gradient_is_bitwise_reproducible():
    """two backward passes from identical dz give torch.equal gradients, for every PointPillar deblock (on deconv_train directly: in
    the whole step the stride-2 layers upstream are not reproducible)"""
    for K, c_up, s in [(64, 128, 1), (128, 128, 2), (256, 128, 4)]:
        x0 = torch.relu(_randn((2, K, 24, 20), 31, 1.0, 0.3)).contiguous(memory_format=CL)
        G = _randn((2, c_up, 24 * s, 20 * s), 32).contiguous(memory_format=CL)
        up = _up(K, c_up, s, 33)
        grads = []
        for _ in range(2):
            x, wt = x0.clone().requires_grad_(), up.weight.detach().clone().requires_grad_()
            (bev_train.deconv_train(x, wt, s, deblock="gemm") * G).sum().backward()
            grads.append((x.grad, wt.grad))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


class _Calls:
    """counts calls of module-level functions (monkeypatched attributes) -> which kernels a step really ran"""

    def __init__(self, monkeypatch, *targets):
        self.n = {}
        for mod, name in targets:
            fn = getattr(mod, name)
            self.n[name] = 0

            def wrapped(*a, _fn=fn, _name=name, **k):
                self.n[_name] += 1
                return _fn(*a, **k)
            monkeypatch.setattr(mod, name, wrapped)

    def take(self):
        out = dict(self.n)
        for k in self.n:
            self.n[k] = 0
        return out


def _fixture_model(z):
    m = BaseBEVBackbone(FIXTURE_CFG, 16)
    sd = {}
    for k, v in m.state_dict().items():
        a = torch.from_numpy(z["bev." + k])
        sd[k] = a.float() * float(z["weight_scale"]) if a.dtype == torch.int8 else a
    m.load_state_dict(sd)
    return m.to(DEV).to(memory_format=CL).train()


def test_backbone_matches_reference_fixture(golden_dir, monkeypatch):
    z = np.load(os.path.join(golden_dir, "deblock_train_ref.npz"))
    x0 = (torch.from_numpy(z["x_code"]).float() * float(z["x_scale"])).to(DEV).contiguous(memory_format=CL)
    G = (torch.from_numpy(z["g_code"]).float() * float(z["g_scale"])).to(DEV).contiguous(memory_format=CL)
    calls = _Calls(monkeypatch, (bev_train, "deconv_forward_gemm"), (bev_train, "deconv_dgrad"), (bev_train, "deconv_wgrad"))
    m = _fixture_model(z)
    tb = bev_train.TrainBEVBackbone(m.blocks, m.deblocks, deblock="gemm")
    assert tb.routes() == ([["conv"], ["conv"], ["conv"]], ["fused"] * 3)
    assert tb.deblock_conv_routes() == [("library", "gemm", "gemm"), ("gemm", "gemm", "gemm"), ("gemm", "gemm", "gemm")]
    x = x0.clone().requires_grad_()
    y = tb(x)
    assert calls.take() == {"deconv_forward_gemm": 2, "deconv_dgrad": 0, "deconv_wgrad": 0}
    assert rel(y, torch.from_numpy(z["out64"]).to(DEV)) < 1e-5
    (y * G).sum().backward()
    assert calls.take() == {"deconv_forward_gemm": 0, "deconv_dgrad": 3, "deconv_wgrad": 3}      # six gradient kernel calls per step
    assert rel(x.grad, torch.from_numpy(z["dx64"]).to(DEV)) < 1e-4
    n_up = 0
    for name, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            assert rel(mod.weight.grad, torch.from_numpy(z["d_gamma." + name]).to(DEV)) < 1e-4, name
            assert rel(mod.bias.grad, torch.from_numpy(z["d_beta." + name]).to(DEV)) < 1e-4, name
        elif isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            key = name + ".weight"
            ref = torch.from_numpy(z["dw16." + key].astype(np.float32)).to(DEV) * float(z["dw_scale." + key])
            assert rel(mod.weight.grad, ref) < 2e-3, name               # float16 storage
            n_up += isinstance(mod, nn.ConvTranspose2d)
    assert n_up == 3
    # the default option runs none of the kernels
    m = _fixture_model(z)
    (bev_train.TrainBEVBackbone(m.blocks, m.deblocks)(x0.clone().requires_grad_()) * G).sum().backward()
    assert calls.take() == {"deconv_forward_gemm": 0, "deconv_dgrad": 0, "deconv_wgrad": 0}


def test_train_loss_gemm_matches_library_option(monkeypatch):
    """the criterion of test_train_loss_fused_matches_stock_and_refolds: every gradient within 10 x the step's own spread under
    2^-17 input noise (the "library" step rerun on a perturbed canvas)"""
    from lidardetection_amd import pillar_ops
    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = pp_inputs(2, 5, 2300)
    models = []
    for _ in range(3):
        torch.manual_seed(6)
        models.append(PointPillarKITTI(batch_size=2, device=DEV).train())
    new, lib, noisy = models
    with pytest.raises(pillar_ops._lib.LidarHipError):
        new.train_loss(pts, offs, gt, backbone="fused", wgrad="wino", deblock="nonsense")
    orig = noisy.backbone_head_train
    noisy.backbone_head_train = lambda c, wgrad="library": orig((c * (1 + NOISE * _randn(c.shape, 9))).contiguous(memory_format=CL), wgrad)
    calls = _Calls(monkeypatch, (bev_train, "deconv_forward_gemm"), (bev_train, "deconv_dgrad"), (bev_train, "deconv_wgrad"))
    lg = new.train_loss(pts, offs, gt, backbone="fused", wgrad="wino", deblock="gemm")
    ll = lib.train_loss(pts, offs, gt, backbone="fused", wgrad="wino")
    ln = noisy.train_loss(pts, offs, gt, backbone="fused", wgrad="wino")
    for a, b in zip(lg, ll):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    sum(lg).backward()
    assert calls.take() == {"deconv_forward_gemm": 2, "deconv_dgrad": 3, "deconv_wgrad": 3}
    for losses in (ll, ln):
        sum(losses).backward()
    assert calls.take() == {"deconv_forward_gemm": 0, "deconv_dgrad": 0, "deconv_wgrad": 0}
    pg, pl, pn = dict(new.named_parameters()), dict(lib.named_parameters()), dict(noisy.named_parameters())
    errs = {k: rel(p.grad, pl[k].grad) for k, p in pg.items() if p.grad is not None and bool(torch.isfinite(p.grad).all())}
    assert len(errs) == len(pl)                                         # every parameter received a finite gradient
    bad = {k: (v, rel(pn[k].grad, pl[k].grad)) for k, v in errs.items() if not v < max(1e-4, 10 * rel(pn[k].grad, pl[k].grad))}
    assert not bad, bad
    tb = new.__dict__["_bev_train_wino_gemm"]                            # the cached backbone is keyed by both options
    assert tb.deblock_conv_routes() == [("library", "gemm", "gemm"), ("gemm", "gemm", "gemm"), ("gemm", "gemm", "gemm")]
    assert "_bev_train_wino" in lib.__dict__ and "_bev_train_wino_gemm" not in lib.__dict__


def test_sync_free():
    torch.manual_seed(12)
    blocks, deblocks = make_bev_backbone()
    base = nn.ModuleList([blocks, deblocks]).to(DEV).to(memory_format=CL).train()
    x0 = torch.relu(_randn((2, 64, 128, 112), 13)).contiguous(memory_format=CL)
    G = _randn((2, 384, 64, 56), 14).contiguous(memory_format=CL)
    for rep in range(3):                                                # rep 0 warms the libraries and the workspaces up outside the check
        mods = copy.deepcopy(base)
        x = x0.clone().requires_grad_()
        tb = bev_train.TrainBEVBackbone(mods[0], mods[1], wgrad="wino", deblock="gemm")
        with no_host_sync(rep > 0):
            (tb(x) * G).sum().backward()
        assert x.grad is not None
    for p in mods.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
