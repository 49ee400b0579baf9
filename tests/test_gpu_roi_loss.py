"""GPU tests of the fused RoI-head loss (csrc/roi_loss.hip, lidardetection_amd/roi_loss.py, the pcdet.models.roi_heads mirror,
PVRCNNKitti.rcnn_loss) against the reference's own float64 run of get_loss (tests/golden/roi_loss_ref.npz) and, over the declared
shapes, against the float64 restatement tests/_roi_loss_torch.py that tests/test_roi_loss_host.py pins to that run.

Tolerances.  cls loss, reg loss: 1e-5 relative; rcnn_cls gradient: 1e-5 x max |gradient| (the bars of tests/test_gpu_anchor_loss.py).
Corner loss and rcnn_reg gradient: the larger of those bars and twice the error of the reference's own float32 run against its
float64 run on the same case (both in the fixture; the factor 2 covers a different, equally valid summation order).  The raw-ABI
sweep has no float32 reference run and uses the project bars alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _gpu_util import no_host_sync
import _roi_loss_torch as rlt
from lidardetection_amd import _lib, roi_loss
from lidardetection_amd.pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from lidardetection_amd.pcdet.utils.cfg import AttrDict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UP = (0.3, 1.7, 0.6)      # upstream gradients of cls, reg, corner
TARGET = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
              CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)


@pytest.fixture(scope="module")
def files():
    return np.load(os.path.join(GOLDEN, "proposal_target_ref.npz")), np.load(os.path.join(GOLDEN, "roi_loss_ref.npz"))


def _case(name, files, dev):
    ptz, rz = files
    t = rlt.case_targets(name, ptz)
    cls, reg = rlt.case_predictions(name, rz)
    td = {k: torch.from_numpy(v).to(dev) for k, v in t.items()}
    return t, td, torch.from_numpy(cls).to(dev).requires_grad_(True), torch.from_numpy(reg).to(dev).requires_grad_(True)


def _bars(name, rz, t):
    """-> (reference losses [cls, reg, corner], expected (d_cls, d_reg) under UP, bars dict) from the fixture's two runs"""
    exp = {}
    for run in (32, 64):
        gcls, greg, gtot = rlt.fixture_grads(name, rz, run, t)
        exp[run] = (UP[0] * gcls, UP[1] * greg + UP[2] * (gtot - greg))
    l32, l64 = rz[f"{name}_loss32"], rz[f"{name}_loss64"]
    gmax = np.abs(exp[64][1]).max()
    bars = dict(cls=1e-5 * abs(l64[0]), reg=1e-5 * abs(l64[1]), corner=max(1e-5 * abs(l64[2]), 2 * abs(l32[2] - l64[2])),
                d_cls=1e-5 * np.abs(exp[64][0]).max(), d_reg=max(1e-5 * gmax, 2 * np.abs(exp[32][1] - exp[64][1]).max()),
                ref32_corner=abs(l32[2] - l64[2]), ref32_d_reg=np.abs(exp[32][1] - exp[64][1]).max(), d_reg_max=gmax)
    return l64, exp[64], bars


@pytest.mark.parametrize("name", list(rlt.CASES))
def test_fixture_case_against_the_reference_float64_run(files, dev, name):
    t, td, x, r = _case(name, files, dev)
    spec = roi_loss.spec_from_cfg(dict(LOSS_CONFIG=rlt.CASES[name][2]))
    cls, reg, cor, stats = roi_loss.roi_head_loss(x, r, td, spec)
    (UP[0] * cls + UP[1] * reg + UP[2] * cor).backward()
    l64, (e_cls, e_reg), bars = _bars(name, files[1], t)
    got = [float(v) for v in (cls, reg, cor)]
    d_cls, d_reg = x.grad.cpu().numpy().astype(np.float64), r.grad.cpu().numpy().astype(np.float64)
    err = dict(cls=abs(got[0] - l64[0]), reg=abs(got[1] - l64[1]), corner=abs(got[2] - l64[2]), d_cls=np.abs(d_cls - e_cls).max(),
               d_reg=np.abs(d_reg - e_reg).max())
    print(f"roi_loss {name}: " + ", ".join(f"{k} err {err[k]:.3e} bar {bars[k]:.3e}" for k in err) +
          f"; reference float32 run: corner err {bars['ref32_corner']:.3e}, d_reg err {bars['ref32_d_reg']:.3e} (max |d_reg| {bars['d_reg_max']:.3e})")
    for k in err:
        assert err[k] <= bars[k], (name, k, err[k], bars[k])
    fg, valid = int((t["reg_valid_mask"] > 0).sum()), int((t["rcnn_cls_labels"] >= 0).sum())
    assert stats.tolist()[3:] == [fg, valid] and stats.tolist()[:3] == got
    # exact zeros wherever the reference's float64 gradients are exactly zero
    assert not d_cls[e_cls == 0].any() and not d_reg[e_reg == 0].any()
    assert np.isfinite(d_cls).all() and np.isfinite(d_reg).all()
    z = rlt.zero_row(name, t)
    if z is not None:
        assert not d_reg[z].any()
    if name in ("nofg", "nocorner"):
        assert got[2] == 0.0
    # the inputs are never written
    for k, v in t.items():
        assert np.array_equal(td[k].cpu().numpy(), v, equal_nan=True), k


def _head(cfg):
    return RoIHeadTemplate(3, AttrDict(TARGET_CONFIG=AttrDict(TARGET, BOX_CODER="ResidualCoder"), LOSS_CONFIG=AttrDict(cfg)))


@pytest.mark.parametrize("name", ["pv", "cls", "nofg", "nocorner"])
def test_mirror_get_loss_keys_and_values(files, dev, name):
    t, td, x, r = _case(name, files, dev)
    head = _head(rlt.CASES[name][2])
    head.forward_ret_dict = dict(td, rcnn_cls=x, rcnn_reg=r)
    loss, tb = head.get_loss()
    ref = json.loads(str(files[1][f"{name}_tb64"]))
    assert list(tb) == list(ref) and ("rcnn_loss_corner" in tb) == (name in ("pv", "cls"))
    l64, _, bars = _bars(name, files[1], t)
    tol = dict(rcnn_loss_cls=bars["cls"], rcnn_loss_reg=bars["reg"], rcnn_loss_corner=bars["corner"],
               rcnn_loss=bars["cls"] + bars["reg"] + bars["corner"])
    for k in ref:
        assert abs(tb[k] - ref[k]) <= tol[k], (name, k, tb[k], ref[k])
    assert abs(float(loss) - ref["rcnn_loss"]) <= tol["rcnn_loss"] + 1e-6 * abs(ref["rcnn_loss"])
    # the two layer losses keep the reference's return shapes: (tensor, its tb entries); the reg loss carries the corner term
    reg_loss, reg_tb = head.get_box_reg_layer_loss(head.forward_ret_dict)
    cls_loss, cls_tb = head.get_box_cls_layer_loss(head.forward_ret_dict)
    assert list(cls_tb) == ["rcnn_loss_cls"] and list(reg_tb) == [k for k in ref if k in ("rcnn_loss_reg", "rcnn_loss_corner")]
    assert abs(float(reg_loss) - (l64[1] + l64[2])) <= bars["reg"] + bars["corner"] and abs(float(cls_loss) - l64[0]) <= bars["cls"]


def test_mirror_torch_fallback_agrees_with_the_fused_path(files, dev):
    t, td, x, r = _case("pv", files, dev)
    l64, (e_cls, e_reg), bars = _bars("pv", files[1], t)
    out = {}
    for kind in ("fused", "torch"):
        head = _head(rlt.PV_LOSS)
        if kind == "torch":
            head._loss_spec = (None,)
        xx, rr = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
        head.forward_ret_dict = dict(td, rcnn_cls=xx, rcnn_reg=rr)
        cls, reg, cor, _ = head._terms(head.forward_ret_dict)
        (UP[0] * cls + UP[1] * reg + UP[2] * cor).backward()
        _, tb = head.get_loss()
        out[kind] = ([float(cls), float(reg), float(cor)], xx.grad.cpu().numpy(), rr.grad.cpu().numpy(), tb)
    for kind, (losses, d_cls, d_reg, tb) in out.items():       # each within the bar of the same float64 value
        for got, exp, k in zip(losses, l64, ("cls", "reg", "corner")):
            assert abs(got - exp) <= bars[k], (kind, k, got, exp)
        assert np.abs(d_cls - e_cls).max() <= bars["d_cls"] and np.abs(d_reg - e_reg).max() <= bars["d_reg"], kind
    assert list(out["fused"][3]) == list(out["torch"][3])
    # a config the fused path refuses runs the torch formulation: CrossEntropy over two columns
    head = _head(dict(rlt.PV_LOSS, CLS_LOSS="CrossEntropy"))
    assert head.build_losses() is None
    lab = (td["rcnn_cls_labels"] > 0.5).long()
    head.forward_ret_dict = dict(td, rcnn_cls_labels=lab, rcnn_cls=torch.cat([-x.detach(), x.detach()], 1) / 2, rcnn_reg=r.detach())
    loss, tb = head.get_loss()
    exp = torch.nn.functional.binary_cross_entropy_with_logits(x.detach().double().reshape(-1), lab.double().reshape(-1))
    assert abs(tb["rcnn_loss_cls"] - float(exp)) <= 1e-5 * float(exp) and abs(tb["rcnn_loss_reg"] - l64[1]) <= bars["reg"]


# ------------------------------------------------------------------------------------------------ raw ABI over the declared shapes
def _random_case(B, P, fg_kind, seed, dev):
    g = torch.Generator().manual_seed(seed)
    n = B * P
    u = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    rois = torch.cat([u(n, 2) * 80 - 40, u(n, 1) * 2 - 2, 1 + u(n, 3) * 3, u(n, 1) * 16 - 8], 1)
    # gts near their rois; heading within 0.4 of the roi's or of its opposite, so no corner sits near a tie of the two distances
    src = torch.cat([rois[:, :3] + (u(n, 3) - 0.5), rois[:, 3:6] * (0.8 + 0.4 * u(n, 3)),
                     rois[:, 6:7] + (u(n, 1) - 0.5) * 0.8 + np.pi * (u(n, 1) < 0.5), u(n, 1)], 1)
    gt = torch.cat([(u(n, 3) - 0.5), src[:, 3:6], (u(n, 1) - 0.5) * 0.8, src[:, 7:8]], 1)
    mask = torch.zeros(n, dtype=torch.int64)
    if fg_kind == "one":
        mask[n // 2] = 1
    elif fg_kind == "all":
        mask[:] = 1
    labels = torch.where(u(n) < 0.2, torch.full((n,), -1.0), u(n))
    x = torch.randn(n, 1, generator=g) * 4
    r = torch.randn(n, 7, generator=g) * torch.tensor([0.3, 0.3, 0.3, 0.15, 0.15, 0.15, 0.1])
    shape = lambda v, w: v.reshape(B, P, w).contiguous().to(dev)      # noqa: E731
    return (x.to(dev), r.to(dev), shape(rois, 7), shape(gt, 8), shape(src, 8), mask.reshape(B, P).to(dev),
            labels.reshape(B, P).to(dev))


SWEEP_W, SWEEP_CW = (1.5, 0.75, 0.5), (1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.3)


@pytest.mark.parametrize("fg_kind", ["none", "one", "all"])
@pytest.mark.parametrize("B,P", [(1, 1), (1, 63), (1, 64), (2, 65), (3, 257), (16, 512)])
def test_raw_abi_sweep_against_the_float64_restatement(dev, B, P, fg_kind):
    x, r, rois, gt, src, mask, labels = _random_case(B, P, fg_kind, 1000 * B + P, dev)
    n, L, G = B * P, _lib.lib(), 64
    keep = [t.clone() for t in (x, r, rois, gt, src, mask, labels)]
    xd, rd = x.double().requires_grad_(True), r.double().requires_grad_(True)
    (cls, reg, cor), (fg_sum, n_valid) = rlt.roi_loss(xd, rd, rois, gt, src, mask, labels, SWEEP_W, SWEEP_CW, True)
    (UP[0] * cls + UP[1] * reg + UP[2] * cor).backward()
    ws = torch.empty(roi_loss.workspace_bytes(B, P), dtype=torch.uint8, device=dev)
    guard = 12345.0
    rec = torch.full((5 + 2 * G,), guard, device=dev)
    d_cls, d_reg = torch.full((n + 2 * G,), guard, device=dev), torch.full((n * 7 + 2 * G,), guard, device=dev)
    grad = torch.tensor(UP, device=dev)
    w, cw = _lib.host_f32(SWEEP_W), _lib.host_f32(SWEEP_CW)
    off = lambda t, k: C.c_void_p(t.data_ptr() + 4 * k)      # noqa: E731
    assert L.lidar_roi_loss_forward(_lib.ptr(x), _lib.ptr(r), _lib.ptr(rois), _lib.ptr(gt), _lib.ptr(src), _lib.ptr(mask),
                                    _lib.ptr(labels), B, P, w, cw, 1, off(rec, G), _lib.ptr(ws), ws.numel(), _lib.stream()) == 0
    assert L.lidar_roi_loss_backward(B, P, w, cw, 1, _lib.ptr(grad), off(d_cls, G), off(d_reg, G), _lib.ptr(ws), ws.numel(),
                                     _lib.stream()) == 0
    torch.cuda.synchronize()
    for t in (rec, d_cls, d_reg):
        assert (t[:G] == guard).all() and (t[-G:] == guard).all(), "a guard band was written"
    for a, b in zip(keep, (x, r, rois, gt, src, mask, labels)):
        assert torch.equal(a, b), "an input was written"
    got = rec[G:G + 5].tolist()
    assert got[3:] == [int(fg_sum), int(n_valid)]
    for g_, e in zip(got[:3], (cls, reg, cor)):
        assert abs(g_ - float(e)) <= 1e-5 * abs(float(e)), (got, float(cls), float(reg), float(cor))
    e_cls, e_reg = xd.grad.reshape(-1), rd.grad.reshape(-1)
    assert (d_cls[G:-G].double() - e_cls).abs().max() <= 1e-5 * e_cls.abs().max()
    assert (d_reg[G:-G].double() - e_reg).abs().max() <= 1e-5 * max(float(e_reg.abs().max()), 1e-30)
    assert not d_reg[G:-G][e_reg == 0].any() and not d_cls[G:-G][e_cls == 0].any()
    # either gradient pointer may be NULL: the other output is the same, the skipped one is untouched
    only = torch.full_like(d_reg, guard)
    assert L.lidar_roi_loss_backward(B, P, w, cw, 1, _lib.ptr(grad), None, off(only, G), _lib.ptr(ws), ws.numel(), _lib.stream()) == 0
    assert torch.equal(only, d_reg)
    only = torch.full_like(d_cls, guard)
    assert L.lidar_roi_loss_backward(B, P, w, cw, 1, _lib.ptr(grad), off(only, G), None, _lib.ptr(ws), ws.numel(), _lib.stream()) == 0
    assert torch.equal(only, d_cls)


def test_empty_batch_and_python_refusals(dev):
    spec = roi_loss.spec_from_cfg(dict(LOSS_CONFIG=rlt.PV_LOSS))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    td = dict(rois=z(0, 128, 7), gt_of_rois=z(0, 128, 8), gt_of_rois_src=z(0, 128, 8), reg_valid_mask=z(0, 128, dt=torch.int64),
              rcnn_cls_labels=z(0, 128))
    cls, reg, cor, stats = roi_loss.roi_head_loss(z(0, 1), z(0, 7), td, spec)
    assert stats.tolist() == [0.0] * 5 and float(cls + reg + cor) == 0.0
    td = dict(rois=z(1, 4, 7), gt_of_rois=z(1, 4, 8), gt_of_rois_src=z(1, 4, 8), reg_valid_mask=z(1, 4, dt=torch.int64),
              rcnn_cls_labels=z(1, 4))
    for bad in (dict(rcnn_reg=z(4, 21)), dict(rcnn_cls=z(4, 3)), dict(rois=z(1, 4, 9)), dict(gt_of_rois=z(1, 4, 10), gt_of_rois_src=z(1, 4, 10)),
                dict(reg_valid_mask=z(1, 4)), dict(rcnn_reg=z(4, 7, dt=torch.float64))):
        args = dict(td, rcnn_cls=z(4, 1), rcnn_reg=z(4, 7))
        args.update(bad)
        with pytest.raises(_lib.LidarHipError):
            roi_loss.roi_head_loss(args.pop("rcnn_cls"), args.pop("rcnn_reg"), args, spec)


def test_sync_free_and_bitwise_deterministic(files, dev):
    t, td, x, r = _case("pv", files, dev)
    spec = roi_loss.spec_from_cfg(dict(LOSS_CONFIG=rlt.PV_LOSS))
    runs = []
    torch.cuda.synchronize()
    for _ in range(2):
        leaves = [v.detach().clone().requires_grad_() for v in (x, r)]
        with no_host_sync():
            cls, reg, cor, stats = roi_loss.roi_head_loss(leaves[0], leaves[1], td, spec)
            (cls + reg + cor).backward()
        runs.append([stats.clone()] + [v.grad.clone() for v in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


def test_pvrcnn_rcnn_targets_into_rcnn_loss(dev):
    """end to end on a small synthetic batch: PVRCNNKitti.rcnn_targets' dict goes into rcnn_loss, eagerly and in a hipGraph"""
    from lidardetection_amd.pvrcnn import PVRCNNKitti
    m = PVRCNNKitti.__new__(PVRCNNKitti)      # the two methods read num_class alone: no trunk is built
    torch.nn.Module.__init__(m)
    m.num_class = 3
    g = torch.Generator().manual_seed(5)
    B, R, M = 2, 96, 6
    gt = torch.zeros(B, M, 8)
    gt[:, :4] = torch.cat([torch.rand(B, 4, 2, generator=g) * 60 - 30, torch.rand(B, 4, 1, generator=g) - 1.5,
                           torch.tensor([3.9, 1.6, 1.56]).expand(B, 4, 3), torch.rand(B, 4, 1, generator=g) * 6 - 3,
                           torch.randint(1, 4, (B, 4, 1), generator=g).float()], -1)
    src = gt[:, torch.arange(R) % 4]
    rois = src[..., :7] + torch.randn(B, R, 7, generator=g) * torch.tensor([0.4, 0.2, 0.1, 0.1, 0.05, 0.05, 0.1]) * (torch.arange(R) % 3)[None, :, None]
    rois, gt = rois.to(dev), gt.to(dev)
    roi_labels, roi_scores = src[..., 7].long().to(dev), torch.rand(B, R, generator=g).to(dev)
    fg_keys, draws = torch.rand(B, R, generator=g).to(dev), torch.rand(B, 128, generator=g).to(dev)
    targets = m.rcnn_targets(rois, roi_scores, roi_labels, gt, fg_keys=fg_keys, draws=draws)
    n = B * 128
    x = (torch.randn(n, 1, generator=g) * 2).to(dev).requires_grad_(True)
    r = (torch.randn(n, 7, generator=g) * 0.1).to(dev).requires_grad_(True)
    loss, stats = m.rcnn_loss(x, r, targets)
    loss.backward()
    rec = stats.tolist()
    assert rec[3] == int((targets["reg_valid_mask"] > 0).sum()) > 0 and rec[4] == int((targets["rcnn_cls_labels"] >= 0).sum()) > 0
    xd, rd = x.detach().double().requires_grad_(True), r.detach().double().requires_grad_(True)
    (cls, reg, cor), _ = rlt.roi_loss(xd, rd, *(targets[k] for k in rlt.TARGET_KEYS), *rlt.case_weights(rlt.PV_LOSS))
    (cls + reg + cor).backward()
    assert abs(float(loss) - float(cls + reg + cor)) <= 1e-5 * float(cls + reg + cor)
    assert (x.grad.double() - xd.grad).abs().max() <= 1e-5 * xd.grad.abs().max()
    assert (r.grad.double() - rd.grad).abs().max() <= 1e-5 * rd.grad.abs().max()
    assert m.rcnn_loss(x, r, targets, loss_config=dict(CORNER_LOSS_REGULARIZATION=False))[1].tolist()[2] == 0.0
    # hipGraph: the forward captures and replays to the same bits
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        m.rcnn_loss(x, r, targets)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        _, captured = m.rcnn_loss(x, r, targets)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int32), stats.view(torch.int32))


def test_mlp_trains_through_the_fused_loss(files, dev):
    """a two-layer MLP producing rcnn_cls / rcnn_reg: parameter gradients through the fused loss vs the float64 restatement"""
    t, td, _, _ = _case("pv", files, dev)
    n = td["reg_valid_mask"].numel()
    torch.manual_seed(3)
    feats = torch.randn(n, 16, device=dev)
    mlp = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8)).to(dev)
    with torch.no_grad():
        mlp[2].weight.mul_(0.3)
    spec = roi_loss.spec_from_cfg(dict(LOSS_CONFIG=rlt.PV_LOSS))
    out = mlp(feats)
    cls, reg, cor, _ = roi_loss.roi_head_loss(out[:, :1], out[:, 1:], td, spec)
    (cls + reg + cor).backward()
    got = [p.grad.double().clone() for p in mlp.parameters()]
    ref = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8)).to(dev).double()
    ref.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
    out = ref(feats.double())
    (cls, reg, cor), _ = rlt.roi_loss(out[:, :1], out[:, 1:], *(td[k] for k in rlt.TARGET_KEYS), *rlt.case_weights(rlt.PV_LOSS))
    (cls + reg + cor).backward()
    for a, p in zip(got, ref.parameters()):
        assert (a - p.grad).abs().max() <= 1e-4 * p.grad.abs().max()
