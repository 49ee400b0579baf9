"""GPU tests of the point-head targets and loss (csrc/point_head.hip, lidardetection_amd/point_head.py, the pcdet.models.dense_heads
mirrors, PVRCNNKitti.point_targets / point_loss) against the reference's own run (tests/golden/point_head_ref.npz) and, over the
declared shapes, against the float64 restatement tests/_point_head_np.py that tests/test_point_head_host.py pins to that run.

Tolerances.  Labels and owners: exact.  Box and part labels: 1e-4 absolute against the float64 run (the project's bar for fp32
geometry).  Losses: 1e-5 relative; gradients: 1e-5 x max |gradient| under the upstream triple UP.  Where a term misses that bar on
a fixture case its bar is the larger of it and twice the error of the reference's own float32 run against its float64 run on the
same case (the rule of tests/test_gpu_roi_loss.py).  The raw-ABI sweep has no float32 reference run and uses the project bars."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _gpu_util import no_host_sync
import _point_head_np as ph
from test_point_head_host import case_loss_inputs, make_head
from lidardetection_amd import _lib, point_head

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UP = (0.3, 1.7, 0.6)      # upstream gradients of cls, box, part
TERMS = ("cls", "box", "part")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "point_head_ref.npz"))


def _spec(name):
    return point_head.spec_from_cfg(ph.CASES[name]["cfg"], ph.CASES[name]["num_class"])


def _check_targets(name, fx, t):
    c = ph.CASES[name]
    assert t["point_cls_labels"].dtype == torch.int64 and t["point_box_idx"].dtype == torch.int32
    assert np.array_equal(t["point_cls_labels"].cpu().numpy(), fx[f"{name}_labels"])
    assert np.array_equal(t["point_box_idx"].cpu().numpy(), fx[f"{name}_owner"])
    for key, on in (("box", c["box"]), ("part", c["part"])):
        got = t[f"point_{key}_labels"]
        if not on:
            assert got is None
            continue
        got, exp = got.cpu().numpy().astype(np.float64), fx[f"{name}_{key}64"]
        assert np.array_equal(np.isnan(got), np.isnan(exp))
        err = np.nanmax(np.abs(got - exp))
        print(f"point_head {name}: {key} labels max err {err:.3e} (bar 1e-4; reference float32 run {np.nanmax(np.abs(fx[f'{name}_{key}32'] - exp)):.3e})")
        assert err <= 1e-4
        assert not got[fx[f"{name}_owner"] < 0].any()      # exact zeros on the rows without an owner


def _bars(name, fx):
    """-> (expected losses, expected gradients under UP, bars) from the fixture's two runs"""
    l32, l64 = fx[f"{name}_loss32"], fx[f"{name}_loss64"]
    exp, bars = {}, {}
    for i, k in enumerate(TERMS):
        bars[k] = max(1e-5 * abs(l64[i]), 2 * abs(l32[i] - l64[i]))
        if f"{name}_g{k}64" in fx:
            g32, g64 = UP[i] * fx[f"{name}_g{k}32"].astype(np.float64), UP[i] * fx[f"{name}_g{k}64"]
            exp[k] = g64
            bars["d_" + k] = max(1e-5 * np.abs(g64).max(), 2 * np.abs(g32 - g64).max())
    return l64, exp, bars


def _loss_inputs(name, fx, dev, targets):
    """predictions as leaves and the targets with the fixture's planted NaN"""
    cls, box, part, *_ = case_loss_inputs(fx, name, "32")
    leaf = lambda a: None if a is None else torch.from_numpy(a).float().to(dev).requires_grad_(True)      # noqa: E731
    t = dict(targets)
    if ph.CASES[name]["box"]:
        r, q = fx[f"{name}_nan"]
        t["point_box_labels"] = t["point_box_labels"].clone()
        t["point_box_labels"][int(r), int(q)] = float("nan")
    return leaf(cls), leaf(box), leaf(part), t


def _check_loss(name, fx, losses, grads, stats):
    l64, exp, bars = _bars(name, fx)
    got = [float(v) for v in losses]
    err = {k: abs(got[i] - l64[i]) for i, k in enumerate(TERMS)}
    for k, g in zip(TERMS, grads):
        if k in exp:
            g = g.cpu().numpy().astype(np.float64)
            err["d_" + k] = np.abs(g - exp[k]).max()
            assert np.isfinite(g).all() and not g[exp[k] == 0].any(), k      # exact zeros where the reference's are
        else:
            assert g is None
    print(f"point_head {name}: " + ", ".join(f"{k} err {err[k]:.3e} bar {bars[k]:.3e}" for k in err))
    for k in err:
        assert err[k] <= bars[k], (name, k, err[k], bars[k])
    assert stats.tolist() == got + [float(fx[f"{name}_pos"])]


@pytest.mark.parametrize("name", list(ph.CASES))
def test_fixture_case_through_the_public_api(fx, dev, name):
    c, spec = ph.CASES[name], _spec(name)
    pts, gt = torch.from_numpy(fx[f"{name}_points"]).to(dev), torch.from_numpy(fx[f"{name}_gt"]).to(dev)
    t = point_head.assign_point_targets(pts, gt, spec, c["box"], c["part"])
    _check_targets(name, fx, t)
    assert np.array_equal(pts.cpu().numpy(), fx[f"{name}_points"]) and np.array_equal(gt.cpu().numpy(), fx[f"{name}_gt"])
    x, b, p, t = _loss_inputs(name, fx, dev, t)
    cls, box, part, stats = point_head.point_head_loss(x, b, p, t, spec)
    (UP[0] * cls + UP[1] * box + UP[2] * part).backward()
    _check_loss(name, fx, (cls, box, part), [None if v is None else v.grad for v in (x, b, p)], stats)


@pytest.mark.parametrize("name", list(ph.CASES))
def test_fixture_case_through_the_mirror_class(fx, dev, name):
    c = ph.CASES[name]
    head = make_head(name).to(dev)
    assert head.fused_spec() is not None
    pts, gt = torch.from_numpy(fx[f"{name}_points"]).to(dev), torch.from_numpy(fx[f"{name}_gt"]).to(dev)
    t = head.assign_targets({"point_coords": pts, "gt_boxes": gt})
    _check_targets(name, fx, t)
    x, b, p, t = _loss_inputs(name, fx, dev, t)
    ret = {"point_cls_preds": x, "point_cls_labels": t["point_cls_labels"]}
    if c["box"]:
        ret.update(point_box_preds=b, point_box_labels=t["point_box_labels"])
    if c["part"]:
        ret.update(point_part_preds=p, point_part_labels=t["point_part_labels"])
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    ref = json.loads(str(fx[f"{name}_tb64"]))
    _, _, bars = _bars(name, fx)
    assert list(tb) == list(ref) and tb["point_pos_num"] == ref["point_pos_num"]
    for k in TERMS:
        if "point_loss_" + k in ref:
            assert abs(tb["point_loss_" + k] - ref["point_loss_" + k]) <= bars[k], (k, tb, ref)
    assert abs(float(loss) - sum(fx[f"{name}_loss64"])) <= sum(bars[k] for k in TERMS) + 1e-6 * abs(float(loss))
    cls, box, part, stats = head._terms()
    x.grad = None
    (UP[0] * cls + UP[1] * box + UP[2] * part).backward()
    _check_loss(name, fx, (cls, box, part), [None if v is None else v.grad for v in (x, b, p)], stats)


def test_mirror_with_extend_gt_boxes_from_the_caller(fx, dev):
    """boxes the caller enlarged itself take the torch formulation (their content is used, whatever became of the tensor on the
    way) and give the fused path's labels when they are enlarged by the config's widths; other widths give other labels"""
    name = "parta2_box"
    head = make_head(name).to(dev)
    pts, gt = torch.from_numpy(fx[f"{name}_points"]).to(dev), torch.from_numpy(fx[f"{name}_gt"]).to(dev)
    ext = gt.clone()
    ext[..., 3:6] += gt.new_tensor(ph.CASES[name]["cfg"]["TARGET_CONFIG"]["GT_EXTRA_WIDTH"])
    t = head.assign_stack_targets(pts, gt, extend_gt_boxes=ext.clone().contiguous(), ret_box_labels=True, ret_part_labels=True)
    assert np.array_equal(t["point_cls_labels"].cpu().numpy(), fx[f"{name}_labels"])
    assert np.array_equal(t["point_box_idx"].cpu().numpy(), fx[f"{name}_owner"])
    assert np.nanmax(np.abs(t["point_part_labels"].cpu().numpy() - fx[f"{name}_part64"])) <= 1e-4
    wide = gt.clone()
    wide[..., 3:6] += 2.0
    t2 = head.assign_stack_targets(pts, gt, extend_gt_boxes=wide)
    assert int((t2["point_cls_labels"] == -1).sum()) > int((fx[f"{name}_labels"] == -1).sum())


# ------------------------------------------------------------------------------------------------ raw ABI over the declared shapes
GUARD = 64


class Guarded:
    """a device buffer with GUARD elements of a sentinel on each side of the part the kernel may write"""

    def __init__(self, shape, dtype, dev, sentinel):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev)
        self.view, self.shape, self.sentinel = self.full[GUARD:GUARD + n], shape, sentinel

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def get(self):
        g = torch.cat([self.full[:GUARD], self.full[GUARD + self.view.numel():]])
        assert bool((g == self.sentinel).all()), "a write outside the output"
        return self.view.reshape(self.shape).cpu().numpy()


def _raw_targets(L, dev, pts, gt, num_class, mean, flags):
    N, (B, M) = len(pts), gt.shape[:2]
    d_pts, d_gt = torch.from_numpy(pts).to(dev), torch.from_numpy(gt).to(dev)
    lab, own = Guarded((N,), torch.int64, dev, -77), Guarded((N,), torch.int32, dev, -77)
    box, part = Guarded((N, 8), torch.float32, dev, -77.0), Guarded((N, 3), torch.float32, dev, -77.0)
    st = L.lidar_point_targets(_lib.ptr(d_pts), N, _lib.ptr(d_gt), B, M, 8, _lib.host_f32(ph.EXTRA), num_class, flags,
                               _lib.host_f32(np.ravel(mean)) if mean is not None else None, 0 if mean is None else len(mean),
                               lab.ptr(), box.ptr() if flags & 1 else None, part.ptr() if flags & 2 else None, own.ptr(), _lib.stream())
    assert st == 0
    return lab, own, box, part


@pytest.mark.parametrize("N,M,B,num_class,positives,seed", list(ph.sweep_cases()))
def test_raw_abi_sweep_against_the_restatement(dev, N, M, B, num_class, positives, seed):
    L = _lib.lib()
    pts, gt, _ = ph.sweep_inputs(seed, N, M, B, num_class, positives)
    mean = ph.MEAN_SIZE if num_class == 3 else None
    lab, own, box, part = _raw_targets(L, dev, pts, gt, num_class, mean, 3)
    exp = ph.targets(pts, gt, ph.EXTRA, num_class, mean, True, True)
    labels = lab.get()
    assert np.array_equal(labels, exp["labels"]) and np.array_equal(own.get(), exp["owner"])
    g_box, g_part = box.get(), part.get()
    assert np.abs(g_box - exp["box"]).max() <= 1e-4 and np.abs(g_part - exp["part"]).max() <= 1e-4
    assert not g_box[exp["owner"] < 0].any() and not g_part[exp["owner"] < 0].any()
    # the loss on these targets: all three terms, then with NULL predictions and NULL gradients
    r = np.random.default_rng(seed)
    preds = [r.normal(0, 2, (N, num_class)).astype(np.float32), (g_box + r.normal(0, 0.12, (N, 8))).astype(np.float32),
             r.normal(0, 2, (N, 3)).astype(np.float32)]
    weights, cw = [1.5, 0.5, 2.0], [1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 1.25]
    d_lab, d_boxl, d_partl = (torch.from_numpy(a).to(dev) for a in (labels, g_box, g_part))
    d_pred = [torch.from_numpy(a).to(dev) for a in preds]
    grad = torch.tensor(UP, dtype=torch.float32, device=dev)
    nbytes = L.lidar_point_loss_ws_bytes(N)
    assert nbytes > 0
    for present in ((1, 1, 1), (1, 0, 0), (0, 1, 1)):
        ws, out = Guarded((nbytes,), torch.uint8, dev, 0xAB), Guarded((4,), torch.float32, dev, -77.0)
        pp = [_lib.ptr(d) if on else None for d, on in zip(d_pred, present)]
        args = (*pp, _lib.ptr(d_lab), _lib.ptr(d_boxl), _lib.ptr(d_partl), N, num_class, _lib.host_f32(weights), _lib.host_f32(cw))
        assert L.lidar_point_loss_forward(*args, out.ptr(), ws.ptr(), nbytes, _lib.stream()) == 0
        outs = [Guarded(p.shape, torch.float32, dev, -77.0) for p in preds]
        assert L.lidar_point_loss_backward(*args, _lib.ptr(grad), *[o.ptr() if on else None for o, on in zip(outs, present)], ws.ptr(),
                                           nbytes, _lib.stream()) == 0
        e_loss, e_pos, e_grads = ph.loss(*[p if on else None for p, on in zip(preds, present)], labels, g_box, g_part, num_class, weights, cw)
        rec = out.get()
        ws.get()
        assert rec[3] == e_pos == int((exp["labels"] > 0).sum())
        for i in range(3):
            assert abs(rec[i] - e_loss[i]) <= 1e-5 * abs(e_loss[i]) + 1e-30, (i, rec[i], e_loss[i])
            if present[i]:
                g, e = outs[i].get().astype(np.float64), UP[i] * e_grads[i]
                assert np.abs(g - e).max() <= 1e-5 * np.abs(e).max() + 1e-30, (i, np.abs(g - e).max(), np.abs(e).max())
                assert not g[e == 0].any()
            else:
                assert rec[i] == 0.0 and bool((outs[i].full == -77.0).all())      # a NULL pointer: nothing written


def test_no_points_and_no_gts(dev):
    spec = _spec("parta2_box")
    gt = torch.from_numpy(np.load(os.path.join(GOLDEN, "point_head_ref.npz"))["pv_gt"]).to(dev)
    t = point_head.assign_point_targets(torch.zeros((0, 4), device=dev), gt, spec, True, True)
    assert t["point_cls_labels"].shape == (0,) and t["point_box_labels"].shape == (0, 8) and t["point_part_labels"].shape == (0, 3)
    x = torch.zeros((0, 3), device=dev, requires_grad=True)
    cls, box, part, stats = point_head.point_head_loss(x, torch.zeros((0, 8), device=dev), torch.zeros((0, 3), device=dev), t, spec)
    assert stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    (cls + box + part).backward()
    assert x.grad.shape == (0, 3)
    pts = torch.from_numpy(ph.sweep_inputs(1, 300, 4, 2, 3, "all")[0]).to(dev)
    t = point_head.assign_point_targets(pts, torch.zeros((2, 0, 8), device=dev), spec, True, True)
    assert not t["point_cls_labels"].any() and bool((t["point_box_idx"] == -1).all())
    assert not t["point_box_labels"].any() and not t["point_part_labels"].any()
    x = torch.randn((300, 3), device=dev, requires_grad=True)
    cls, box, part, stats = point_head.point_head_loss(x, None, None, t, spec)
    e_loss, _, _ = ph.loss(x.detach().cpu().numpy(), None, None, np.zeros(300, np.int64), None, None, 3, [2.0, 0.5, 1.5], [1.0] * 8)
    assert abs(float(cls) - e_loss[0]) <= 1e-5 * e_loss[0] and stats.tolist()[1:] == [0.0, 0.0, 0.0]


def test_two_calls_are_bit_equal(fx, dev):
    name, runs = "parta2_box", []
    spec = _spec(name)
    pts, gt = torch.from_numpy(fx[f"{name}_points"]).to(dev), torch.from_numpy(fx[f"{name}_gt"]).to(dev)
    for _ in range(2):
        t = point_head.assign_point_targets(pts, gt, spec, True, True)
        x, b, p, tt = _loss_inputs(name, fx, dev, t)
        cls, box, part, stats = point_head.point_head_loss(x, b, p, tt, spec)
        (UP[0] * cls + UP[1] * box + UP[2] * part).backward()
        runs.append([t[k].cpu().numpy() for k in sorted(t)] + [stats.cpu().numpy()] + [v.grad.cpu().numpy() for v in (x, b, p)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_no_host_synchronisation(fx, dev):
    name = "parta2_box"
    spec = _spec(name)
    pts, gt = torch.from_numpy(fx[f"{name}_points"]).to(dev), torch.from_numpy(fx[f"{name}_gt"]).to(dev)
    t = point_head.assign_point_targets(pts, gt, spec, True, True)      # warm: library loaded, allocator primed
    x, b, p, tt = _loss_inputs(name, fx, dev, t)
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    with no_host_sync():
        t2 = point_head.assign_point_targets(pts, gt, spec, True, True)
        cls, box, part, stats = point_head.point_head_loss(x, b, p, tt, spec)
        (up[0] * cls + up[1] * box + up[2] * part).backward()
    assert torch.equal(t2["point_cls_labels"], t["point_cls_labels"]) and x.grad is not None and b.grad is not None and p.grad is not None


def test_pvrcnn_point_targets_and_loss_equal_the_mirror(dev):
    from lidardetection_amd.pvrcnn import PVRCNNKitti
    B, K = 2, 300
    pts, gt, _ = ph.sweep_inputs(11, B * K, 9, B, 1, "mixed")
    order = np.argsort(pts[:, 0], kind="stable")
    pts = pts[order][:B * K]
    per = min((pts[:, 0] == b).sum() for b in range(B))
    kp = np.stack([pts[pts[:, 0] == b][:per, 1:4] for b in range(B)])
    kp_d, gt_d = torch.from_numpy(kp).to(dev), torch.from_numpy(gt).to(dev)
    model = PVRCNNKitti.__new__(PVRCNNKitti)      # the two methods read no module state
    t = PVRCNNKitti.point_targets(model, kp_d, gt_d)
    head = make_head("pv").to(dev)
    flat = torch.cat([torch.arange(B, device=dev, dtype=torch.float32).repeat_interleave(per).unsqueeze(1), kp_d.reshape(-1, 3)], 1)
    tm = head.assign_targets({"point_coords": flat, "gt_boxes": gt_d})
    assert torch.equal(t["point_cls_labels"], tm["point_cls_labels"]) and torch.equal(t["point_box_idx"], tm["point_box_idx"])
    assert int((t["point_cls_labels"] > 0).sum()) > 0 and int((t["point_cls_labels"] < 0).sum()) > 0
    exp = ph.targets(flat.cpu().numpy(), gt, ph.EXTRA, 1)
    assert np.array_equal(t["point_cls_labels"].cpu().numpy(), exp["labels"])
    x = torch.randn((B * per, 1), device=dev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    loss, stats = PVRCNNKitti.point_loss(model, xa, t)
    head.forward_ret_dict = {"point_cls_preds": xb, "point_cls_labels": tm["point_cls_labels"]}
    loss_m, tb = head.get_loss()
    loss.backward()
    loss_m.backward()
    assert float(loss) == float(loss_m) == tb["point_loss_cls"] and torch.equal(xa.grad, xb.grad) and stats.tolist()[3] == tb["point_pos_num"]


def test_abi_refuses_bad_arguments_without_a_launch(dev):
    L = _lib.lib()
    ERR = -1
    N, B, M = 100, 2, 5
    pts, gt = torch.zeros((N, 4), device=dev), torch.zeros((B, M, 8), device=dev)
    lab, own = Guarded((N,), torch.int64, dev, -77), Guarded((N,), torch.int32, dev, -77)
    box, part = Guarded((N, 8), torch.float32, dev, -77.0), Guarded((N, 3), torch.float32, dev, -77.0)
    ew, mean = _lib.host_f32(ph.EXTRA), _lib.host_f32(np.ravel(ph.MEAN_SIZE))

    def targets(n=N, b=B, m=M, gd=8, nc=3, flags=3, mean=mean, nm=3, ew=ew, p=_lib.ptr(pts), g=_lib.ptr(gt), lp=lab.ptr(), bp=box.ptr(),
                pp=part.ptr(), op=own.ptr()):
        return L.lidar_point_targets(p, n, g, b, m, gd, ew, nc, flags, mean, nm, lp, bp, pp, op, _lib.stream())
    for kw in (dict(n=-1), dict(n=(1 << 20) + 1), dict(b=0), dict(b=65), dict(m=-1), dict(m=129), dict(gd=7), dict(gd=9), dict(nc=0),
               dict(nc=9), dict(nm=9), dict(nm=-1), dict(flags=4), dict(mean=None), dict(ew=None), dict(p=None), dict(g=None),
               dict(lp=None), dict(bp=None), dict(pp=None), dict(op=None)):
        assert targets(**kw) == ERR, kw
    x, xb, xp = torch.zeros((N, 3), device=dev), torch.zeros((N, 8), device=dev), torch.zeros((N, 3), device=dev)
    labels, bl, pl = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros((N, 8), device=dev), torch.zeros((N, 3), device=dev)
    nbytes = L.lidar_point_loss_ws_bytes(N)
    ws, out = Guarded((nbytes,), torch.uint8, dev, 0xAB), Guarded((4,), torch.float32, dev, -77.0)
    w, cw, grad = _lib.host_f32([1, 1, 1]), _lib.host_f32([1] * 8), torch.ones(3, device=dev)
    dc, db, dp = (Guarded(s, torch.float32, dev, -77.0) for s in ((N, 3), (N, 8), (N, 3)))

    def fwd(n=N, nc=3, w=w, cw=cw, lp=_lib.ptr(labels), blp=_lib.ptr(bl), plp=_lib.ptr(pl), o=out.ptr(), wsp=ws.ptr(), nb=nbytes):
        return L.lidar_point_loss_forward(_lib.ptr(x), _lib.ptr(xb), _lib.ptr(xp), lp, blp, plp, n, nc, w, cw, o, wsp, nb, _lib.stream())

    def bwd(n=N, nc=3, w=w, cw=cw, lp=_lib.ptr(labels), blp=_lib.ptr(bl), g=_lib.ptr(grad), wsp=ws.ptr(), nb=nbytes, xbp=_lib.ptr(xb)):
        return L.lidar_point_loss_backward(_lib.ptr(x), xbp, _lib.ptr(xp), lp, blp, _lib.ptr(pl), n, nc, w, cw, g, dc.ptr(), db.ptr(),
                                           dp.ptr(), wsp, nb, _lib.stream())
    for kw in (dict(n=-1), dict(n=(1 << 20) + 1), dict(nc=0), dict(nc=9), dict(w=None), dict(cw=None), dict(lp=None), dict(blp=None),
               dict(plp=None), dict(o=None), dict(wsp=None)):
        assert fwd(**kw) == ERR, kw
    assert fwd(nb=nbytes - 1) == -3
    for kw in (dict(n=-1), dict(nc=9), dict(w=None), dict(cw=None), dict(lp=None), dict(blp=None), dict(g=None), dict(wsp=None), dict(xbp=None)):
        assert bwd(**kw) == ERR, kw
    assert bwd(nb=nbytes - 1) == -3
    torch.cuda.synchronize()
    for g in (lab, own, box, part, ws, out, dc, db, dp):      # nothing was launched: every buffer still holds its sentinel
        assert bool((g.full == g.sentinel).all())
