"""GPU tests of the multi-frame point head and union gt boxes (csrc/point_head_mf.hip, lidardetection_amd/point_head_mf.py, the
PointHeadSimpleMultiFrame mirror) against the reference's own run (tests/golden/point_head_mf_ref.npz) and, over the declared
shapes, against the float64 restatement tests/_point_head_mf_np.py that tests/test_point_head_mf_host.py pins to that run.

Tolerances, those of tests/test_gpu_point_head.py.  Labels and owners: exact.  Loss: 1e-5 relative; gradient: 1e-5 x max |gradient|
under the upstream factor UP; on a fixture case each bar is the larger of that and twice the error of the reference's own float32
run against its float64 run.  Union boxes: 1e-4 absolute against the float64 run (the project's bar for fp32 geometry).  The
raw-ABI sweep has no float32 reference run and uses the project bars."""
import json
import os

import numpy as np
import pytest
import torch

from _gpu_util import no_host_sync
import _point_head_mf_np as mf
from test_gpu_point_head import Guarded
from test_point_head_mf_host import case_inputs, make_head
from lidardetection_amd import _lib, anchor_assign, point_head, point_head_mf

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UP = 0.3      # upstream gradient of the loss


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "point_head_mf_ref.npz"))


def _spec(name):
    return point_head_mf.spec_from_cfg(mf.CASES[name]["cfg"], mf.CASES[name]["num_class"])


def _device_inputs(fx, name, dev):
    pts, gt, loc, rot, x = case_inputs(fx, name)
    return [torch.from_numpy(a).to(dev) for a in (pts, gt, loc, rot)], torch.from_numpy(x).float().to(dev).requires_grad_(True)


def _bars(name, fx):
    l32, l64 = float(fx[f"{name}_loss32"]), float(fx[f"{name}_loss64"])
    g32, g64 = UP * fx[f"{name}_gcls32"].astype(np.float64), UP * fx[f"{name}_gcls64"]
    return l64, g64, max(1e-5 * abs(l64), 2 * abs(l32 - l64)), max(1e-5 * np.abs(g64).max(), 2 * np.abs(g32 - g64).max())


def _check_targets(name, fx, labels, owner):
    assert labels.dtype == torch.int64 and owner.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), fx[f"{name}_labels"]) and np.array_equal(owner.cpu().numpy(), fx[f"{name}_owner"])


def _check_loss(name, fx, loss, grad, stats):
    l64, g64, bar_l, bar_g = _bars(name, fx)
    g = grad.cpu().numpy().astype(np.float64)
    err_l, err_g = abs(float(loss) - l64), np.abs(g - g64).max()
    print(f"point_head_mf {name}: loss err {err_l:.3e} bar {bar_l:.3e}, gradient err {err_g:.3e} bar {bar_g:.3e}")
    assert err_l <= bar_l and err_g <= bar_g
    assert np.isfinite(g).all() and not g[g64 == 0].any()      # exact zeros where the reference's are
    assert stats.tolist() == [float(loss), float(fx[f"{name}_pos"])]


@pytest.mark.parametrize("name", list(mf.CASES))
def test_fixture_case_through_the_public_api(fx, dev, name):
    S, spec = mf.CASES[name]["frames"], _spec(name)
    (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
    t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
    _check_targets(name, fx, t["point_cls_labels_stacked"], t["point_box_idx"])
    assert len(t["point_cls_labels"]) == S and all(torch.equal(c, t["point_cls_labels_stacked"][:, s]) for s, c in enumerate(t["point_cls_labels"]))
    cls, stats = point_head_mf.point_head_loss_mf(x, t, spec, S)
    (UP * cls).backward()
    _check_loss(name, fx, cls.detach(), x.grad, stats)
    # the reference's list alone is enough
    x2 = x.detach().clone().requires_grad_(True)
    cls2, _ = point_head_mf.point_head_loss_mf(x2, {"point_cls_labels": t["point_cls_labels"]}, spec, S)
    (UP * cls2).backward()
    assert float(cls2) == float(cls) and torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize("name", list(mf.CASES))
def test_fixture_case_through_the_mirror_class(fx, dev, name):
    S = mf.CASES[name]["frames"]
    head = make_head(name).to(dev)
    (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
    assert head.fused_spec() is not None and point_head_mf.supported(len(pts), gt.shape[0], gt.shape[1], S, head.num_class)
    t = head.assign_targets({"point_coords": pts, "gt_boxes": gt, "locations": loc, "rotations_y": rot})
    assert isinstance(t, list) and len(t) == S
    _check_targets(name, fx, torch.stack([d["point_cls_labels"] for d in t], 1), torch.stack([d["point_box_idx"] for d in t], 1))
    head.forward_ret_dict = {"point_cls_preds": x, "point_cls_labels": [d["point_cls_labels"] for d in t]}
    loss, tb = head.get_loss()
    ref = json.loads(str(fx[f"{name}_tb64"]))
    _, _, bar_l, _ = _bars(name, fx)
    assert list(tb) == list(ref) and tb["point_pos_num"] == ref["point_pos_num"] and abs(tb["point_loss_cls"] - ref["point_loss_cls"]) <= bar_l
    (UP * loss).backward()
    _check_loss(name, fx, loss.detach(), x.grad, torch.tensor([tb["point_loss_cls"], tb["point_pos_num"]]))
    # the fused path and the torch formulation compute the same loss
    x2 = x.detach().clone().requires_grad_(True)
    cls_t, stats_t = head._torch_terms_mf(x2, torch.stack([d["point_cls_labels"] for d in t], 1))
    assert abs(float(cls_t) - float(loss)) <= 1e-5 * abs(float(loss)) and stats_t.tolist()[1] == tb["point_pos_num"]


def _raw_targets(L, dev, pts, gt, loc, rot, num_class, with_owner=True):
    N, (B, M, S) = len(pts), loc.shape[:3]
    d = [torch.from_numpy(a).to(dev) for a in (pts, gt, loc, rot)]
    keep = [a.clone() for a in d]
    lab, own = Guarded((N, S), torch.int64, dev, -77), Guarded((N, S), torch.int32, dev, -77)
    st = L.lidar_point_targets_mf(_lib.ptr(d[0]), N, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), B, M, S, _lib.host_f32(mf.EXTRA),
                                  num_class, lab.ptr(), own.ptr() if with_owner else None, _lib.stream())
    assert st == 0
    labels, owner = lab.get(), own.get()
    assert all(torch.equal(a, b) for a, b in zip(d, keep)), "an input was written"
    return labels, owner


def _raw_loss(L, dev, x, labels, S, C, weight):
    """-> (record (2), gradient) through the raw ABI with guard bands around every output and the workspace"""
    N = len(labels)
    d_x, d_lab = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    keep = (d_x.clone(), d_lab.clone())
    nbytes = L.lidar_point_loss_mf_ws_bytes(N)
    assert nbytes > 0
    ws, out = Guarded((nbytes,), torch.uint8, dev, 0xAB), Guarded((2,), torch.float32, dev, -77.0)
    grad, dx = torch.tensor([UP], dtype=torch.float32, device=dev), Guarded(x.shape, torch.float32, dev, -77.0)
    assert L.lidar_point_loss_mf_forward(_lib.ptr(d_x), _lib.ptr(d_lab), N, S, C, weight, out.ptr(), ws.ptr(), nbytes, _lib.stream()) == 0
    assert L.lidar_point_loss_mf_backward(_lib.ptr(d_x), _lib.ptr(d_lab), N, S, C, weight, _lib.ptr(grad), dx.ptr(), ws.ptr(), nbytes,
                                          _lib.stream()) == 0
    ws.get()
    assert torch.equal(d_x, keep[0]) and torch.equal(d_lab, keep[1]), "an input was written"
    return out.get(), dx.get()


@pytest.mark.parametrize("name", list(mf.CASES))
def test_fixture_case_through_the_raw_abi(fx, dev, name):
    c = mf.CASES[name]
    pts, gt, loc, rot, x = case_inputs(fx, name)
    labels, owner = _raw_targets(_lib.lib(), dev, pts, gt, loc, rot, c["num_class"])
    assert np.array_equal(labels, fx[f"{name}_labels"]) and np.array_equal(owner, fx[f"{name}_owner"])
    rec, g = _raw_loss(_lib.lib(), dev, x.astype(np.float32), labels, c["frames"], c["num_class"],
                       c["cfg"]["LOSS_CONFIG"]["LOSS_WEIGHTS"]["point_cls_weight"])
    _check_loss(name, fx, rec[0], torch.from_numpy(g), torch.from_numpy(rec))


@pytest.mark.parametrize("name", list(mf.CASES))
def test_each_column_equals_the_single_frame_kernel_on_substituted_boxes(fx, dev, name):
    S, spec = mf.CASES[name]["frames"], _spec(name)
    (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
    t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
    for s in range(S):
        sub = gt.clone()
        sub[..., 0:3], sub[..., 6] = loc[:, :, s], rot[:, :, s]
        one = point_head.assign_point_targets(pts, sub, spec)
        assert torch.equal(t["point_cls_labels"][s], one["point_cls_labels"]) and torch.equal(t["point_box_idx"][:, s], one["point_box_idx"])
    if S == 1:      # one frame: the loss is the single-frame head's
        cls, stats = point_head_mf.point_head_loss_mf(x, t, spec, 1)
        cls.backward()
        x1 = x.detach().clone().requires_grad_(True)
        cls1, _, _, stats1 = point_head.point_head_loss(x1, None, None, {"point_cls_labels": t["point_cls_labels"][0]}, spec)
        cls1.backward()
        assert abs(float(cls) - float(cls1)) <= 1e-6 * abs(float(cls1)) and stats.tolist()[1] == stats1.tolist()[3]
        assert (x.grad - x1.grad).abs().max() <= 1e-6 * x1.grad.abs().max()


@pytest.mark.parametrize("N,M,S,C,B,positives,seed", list(mf.sweep_cases()))
def test_raw_abi_sweep_against_the_restatement(dev, N, M, S, C, B, positives, seed):
    """every output buffer is pre-filled with a sentinel and sits between guard bands: each element is overwritten, nothing
    outside is touched, and the inputs keep their contents"""
    L = _lib.lib()
    pts, gt, loc, rot = mf.sweep_inputs(seed, N, M, S, C, B, positives)
    e_lab, e_own = mf.targets(pts, gt, loc, rot, mf.EXTRA, C)
    labels, owner = _raw_targets(L, dev, pts, gt, loc, rot, C)
    assert np.array_equal(labels, e_lab.reshape(N, S)) and np.array_equal(owner, e_own.reshape(N, S))
    lab2, own2 = _raw_targets(L, dev, pts, gt, loc, rot, C, with_owner=False)      # NULL point_box_idx
    assert np.array_equal(lab2, labels) and (own2 == -77).all()
    x = np.random.default_rng(seed).normal(0, 2, (N, S * C)).astype(np.float32)
    rec, g = _raw_loss(L, dev, x, labels, S, C, 1.5)
    e_loss, e_pos, e_grad = mf.loss(x, labels, C, 1.5)
    assert rec[1] == e_pos and abs(rec[0] - e_loss) <= 1e-5 * abs(e_loss) + 1e-30, (rec, e_loss)
    if N:
        e = UP * e_grad
        assert np.abs(g - e).max() <= 1e-5 * np.abs(e).max() + 1e-30 and not g[e == 0].any()
    if positives == "all" and M and N:
        assert e_pos == N * S
    if positives == "ignored" and M and N:
        assert rec.tolist() == [0.0, 0.0] and not g.any()
    if positives == "none":
        assert e_pos == 0 and (N == 0 or rec[0] > 0)


def test_two_runs_are_bit_equal(fx, dev):
    name, runs = "agnostic3", []
    spec = _spec(name)
    for _ in range(2):
        (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
        t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
        cls, stats = point_head_mf.point_head_loss_mf(x, t, spec, 3)
        (UP * cls).backward()
        e = point_head_mf.enlarged_gt_boxes(gt, loc, rot)
        runs.append([v.cpu().numpy() for v in (t["point_cls_labels_stacked"], t["point_box_idx"], stats, x.grad, e)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    # and at a size with many tiles, where the order of the sums could show
    pts, gt, loc, rot = mf.sweep_inputs(5, 1000, 128, 3, 1, 1, "mixed")
    labels, _ = mf.targets(pts, gt, loc, rot, mf.EXTRA, 1)
    x = np.random.default_rng(5).normal(0, 2, (1000, 3)).astype(np.float32)
    (r1, g1), (r2, g2) = (_raw_loss(_lib.lib(), dev, x, labels, 3, 1, 1.0) for _ in range(2))
    assert r1.tobytes() == r2.tobytes() and g1.tobytes() == g2.tobytes()


def test_inputs_are_never_written_and_no_host_synchronisation(fx, dev):
    name = "classes2"
    spec = _spec(name)
    (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
    keep = [a.clone() for a in (pts, gt, loc, rot, x.detach())]
    t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)      # warm: library loaded, allocator primed
    cls, _ = point_head_mf.point_head_loss_mf(x, t, spec, 2)
    cls.backward()
    point_head_mf.enlarged_gt_boxes(gt, loc, rot)
    x.grad = None
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    with no_host_sync():
        t2 = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
        cls, stats = point_head_mf.point_head_loss_mf(x, t2, spec, 2)
        (up * cls).backward()
        e = point_head_mf.enlarged_gt_boxes(gt, loc, rot)
    assert torch.equal(t2["point_cls_labels_stacked"], t["point_cls_labels_stacked"]) and x.grad is not None and e.shape == gt.shape
    assert all(torch.equal(a, b) for a, b in zip(keep, (pts, gt, loc, rot, x.detach())))


def test_work_runs_on_the_current_stream(fx, dev):
    """on a side stream the results are those of the default stream"""
    name = "agnostic3"
    spec = _spec(name)
    (pts, gt, loc, rot), x = _device_inputs(fx, name, dev)
    t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
    e = point_head_mf.enlarged_gt_boxes(gt, loc)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t2 = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
        cls, stats = point_head_mf.point_head_loss_mf(x, t2, spec, 3)
        e2 = point_head_mf.enlarged_gt_boxes(gt, loc)
    side.synchronize()
    assert torch.equal(t2["point_cls_labels_stacked"], t["point_cls_labels_stacked"]) and torch.equal(e, e2)
    assert stats.tolist()[1] == float(fx[f"{name}_pos"])


def test_no_points_and_no_gts(fx, dev):
    spec = _spec("classes2")
    (pts, gt, loc, rot), _ = _device_inputs(fx, "classes2", dev)
    t = point_head_mf.assign_point_targets_mf(pts[:0], gt, loc, rot, spec)
    assert t["point_cls_labels_stacked"].shape == (0, 2) and t["point_box_idx"].shape == (0, 2) and len(t["point_cls_labels"]) == 2
    x = torch.zeros((0, 4), device=dev, requires_grad=True)
    cls, stats = point_head_mf.point_head_loss_mf(x, t, spec, 2)
    assert stats.tolist() == [0.0, 0.0]
    cls.backward()
    assert x.grad.shape == (0, 4)
    t = point_head_mf.assign_point_targets_mf(pts, gt[:, :0], loc[:, :0], rot[:, :0], spec)
    assert not t["point_cls_labels_stacked"].any() and bool((t["point_box_idx"] == -1).all())
    assert point_head_mf.enlarged_gt_boxes(gt[:, :0], loc[:, :0], rot[:, :0]).shape == (3, 0, 8)


def test_union_boxes_against_the_reference_and_the_unused_rotations(fx, dev):
    gt, loc, rot = (torch.from_numpy(fx[k]).to(dev) for k in ("enl_gt", "enl_loc", "enl_rot"))
    keep = (gt.clone(), loc.clone())
    e = point_head_mf.enlarged_gt_boxes(gt, loc, rot)
    got = e.cpu().numpy()
    err = np.abs(got - fx["enl64"]).max()
    print(f"union boxes: max err {err:.3e} (bar 1e-4; reference float32 run {np.abs(fx['enl32'] - fx['enl64']).max():.3e})")
    assert e.dtype == torch.float32 and err <= 1e-4
    assert np.array_equal(got[..., [0, 1, 2, 5, 6, 7]], fx["enl_gt"][..., [0, 1, 2, 5, 6, 7]])      # these columns are copies
    assert torch.equal(gt, keep[0]) and torch.equal(loc, keep[1])
    # the quirk: rotations_y does not enter
    assert torch.equal(point_head_mf.enlarged_gt_boxes(gt, loc, rot + 0.7), e) and torch.equal(point_head_mf.enlarged_gt_boxes(gt, loc), e)
    # raw ABI with guard bands, at the largest declared shape
    r = np.random.default_rng(3)
    big = np.zeros((64, 128, 8), np.float32)
    big[..., 0:3], big[..., 3:6], big[..., 6] = r.uniform(-40, 40, (64, 128, 3)), r.uniform(0.5, 5, (64, 128, 3)), r.uniform(-7, 7, (64, 128))
    big[r.uniform(size=(64, 128)) < 0.2] = 0
    bloc, _ = mf.moved_poses(r, big, 8)
    out = Guarded((64, 128, 8), torch.float32, dev, -77.0)
    d_gt, d_loc = torch.from_numpy(big).to(dev), torch.from_numpy(bloc).to(dev)
    assert _lib.lib().lidar_multiframe_enlarged_boxes(_lib.ptr(d_gt), _lib.ptr(d_loc), 64, 128, 8, 8, out.ptr(), _lib.stream()) == 0
    assert np.abs(out.get() - mf.enlarged(big, bloc)).max() <= 1e-4


def test_union_boxes_feed_the_anchor_assigner(fx, dev):
    """the union boxes go straight into anchor_assign(..., gt_boxes_enlarged=).  Labels and weights do not depend on them.  Where
    they equal the reference's float32 boxes bit for bit the encoded targets equal those from the reference's boxes; otherwise
    the targets are compared with those from the float64 restatement's boxes: the enlarged boxes enter the code only through
    log(dim_enlarged / dim_anchor) in columns 3 and 4, so a box difference d moves a target by at most d / dim (+ the assigner's own
    1e-6 on its log columns); every other column is bit-equal."""
    gt_np, loc_np = fx["enl_gt"], fx["enl_loc"]
    gt, loc = torch.from_numpy(gt_np).to(dev), torch.from_numpy(loc_np).to(dev)
    ours = point_head_mf.enlarged_gt_boxes(gt, loc)
    names = ["Car", "Pedestrian", "Cyclist"]
    r = np.random.default_rng(8)
    real = gt_np[gt_np[..., 3] > 0]
    anchors = []
    for k in range(3):      # anchors around every real gt, whatever its class
        a = np.repeat(real[:, :7], 3, axis=0)
        a[:, 0:2] += r.normal(0, 0.15, (len(a), 2)).astype(np.float32)
        a[:, 3:6] *= r.uniform(0.9, 1.1, (len(a), 3)).astype(np.float32)
        anchors.append(torch.from_numpy(a).to(dev).contiguous())
    per_loc, out_off, a_total = anchor_assign.output_layout([(1, 1, len(a), 1, 1, 7) for a in anchors], True)

    def assign(enl):
        return anchor_assign.assign(anchors, gt, anchor_assign.class_table(names, names), per_loc, out_off, a_total, [0.6, 0.5, 0.5],
                                    [0.45, 0.35, 0.35], [0, 0, 0], 7, gt_boxes_enlarged=enl)
    l1, t1, w1 = assign(ours)
    l0, t0, w0 = assign(None)
    assert torch.equal(l1, l0) and torch.equal(w1, w0) and int((l1 > 0).sum()) >= 10
    plain = [0, 1, 2, 5, 6]
    assert torch.equal(t1[..., plain], t0[..., plain]) and not torch.equal(t1[..., 3:5], t0[..., 3:5])
    ref32 = torch.from_numpy(fx["enl32"]).to(dev)
    if torch.equal(ours, ref32):
        l2, t2, w2 = assign(ref32)
        assert torch.equal(l1, l2) and torch.equal(t1, t2) and torch.equal(w1, w2)
    else:
        ref64 = torch.from_numpy(mf.enlarged(gt_np, loc_np).astype(np.float32)).to(dev)
        l3, t3, w3 = assign(ref64)
        d = (ours - ref64).abs()[..., 3:5][gt[..., 3] > 0] / ref64[..., 3:5][gt[..., 3] > 0]
        bar = float(d.max()) * 1.01 + 1e-6
        print(f"anchor targets from the union boxes: max diff {float((t1 - t3).abs().max()):.3e}, bar {bar:.3e}")
        assert torch.equal(l1, l3) and torch.equal(w1, w3) and torch.equal(t1[..., plain], t3[..., plain])
        assert float((t1 - t3).abs().max()) <= bar
