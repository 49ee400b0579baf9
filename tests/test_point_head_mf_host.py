"""Host tests of the multi-frame point head and union gt boxes: the float64 restatement tests/_point_head_mf_np.py against the
reference's own run (tests/golden/point_head_mf_ref.npz), the declared support, the wrappers' refusals, and the mirror's torch
formulation on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

from _gpu_util import to_cfg
import _point_head_mf_np as mf
from lidardetection_amd import _lib, point_head_mf
from lidardetection_amd.pcdet.models import dense_heads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "point_head_mf_ref.npz"))


def make_head(name, **kw):
    c = mf.CASES[name]
    args = dict(num_class=c["num_class"], input_channels=4, model_cfg=to_cfg(c["cfg"]), stack_frame_size=c["frames"])
    return dense_heads.PointHeadSimpleMultiFrame(**dict(args, **kw))


def case_inputs(fx, name):
    """-> points, gt, locations, rotations_y, logits (float64) of a fixture case"""
    return (*(fx[f"{name}_{k}"] for k in ("points", "gt", "loc", "rot")), fx[f"{name}_pred_cls"].astype(np.float64) / 64)


def test_the_fixture_holds_the_cases_of_this_module(fx):
    assert json.loads(str(fx["cases"])) == mf.CASES
    assert mf.CASES["agnostic3"]["frames"] == 3 and mf.CASES["classes2"]["num_class"] == 2 and mf.CASES["single"]["frames"] == 1


@pytest.mark.parametrize("name", list(mf.CASES))
def test_restatement_reproduces_the_reference(fx, name):
    c = mf.CASES[name]
    S, C = c["frames"], c["num_class"]
    pts, gt, loc, rot, x = case_inputs(fx, name)
    lab, own = mf.targets(pts, gt, loc, rot, mf.EXTRA, C)
    assert np.array_equal(lab, fx[f"{name}_labels"]) and np.array_equal(own, fx[f"{name}_owner"])
    loss, npos, grad = mf.loss(x, lab, C, c["cfg"]["LOSS_CONFIG"]["LOSS_WEIGHTS"]["point_cls_weight"])
    e_loss, e_grad = float(fx[f"{name}_loss64"]), fx[f"{name}_gcls64"]
    assert npos == int(fx[f"{name}_pos"]) and abs(loss - e_loss) <= 1e-9 * abs(e_loss)
    assert np.abs(grad - e_grad).max() <= 1e-9 * np.abs(e_grad).max() and np.array_equal(grad == 0, e_grad == 0)
    tb = json.loads(str(fx[f"{name}_tb64"]))
    assert list(tb) == ["point_loss_cls", "point_pos_num"] and tb["point_pos_num"] == npos
    # what the fixture was built to hold
    moving, ignored, origin = (int(v) for v in fx[f"{name}_planted"])
    assert lab[moving].tolist() == [1 if C == 1 else int(gt[0, 2, 7]), -1, 0][:S] and own[moving].tolist() == [2, -1, -1][:S]
    assert (lab[ignored] == -1).all() and not grad[ignored].any()
    assert not pts[origin].any() and (own[origin] == 4).all() and not gt[0, 4].any() and not loc[0, 4].any()
    assert lab[pts[:, 0] == 3].tolist() == [[0] * S] and not (pts[:, 0] == 2).any() and gt[2, :, 3].any()
    assert (np.abs(rot) > np.pi).any() and (np.diff(pts[:, 0]) < 0).any()
    over = np.nonzero((own[:, 0] == 0) & (pts[:, 0] == 0))[0]      # the first of two overlapping rows wins
    assert len(over) and (mf.ph.targets(pts[over], mf.substituted(gt, loc, rot, 0)[:, 1:], mf.EXTRA, C)["owner"] == 0).any()
    if S > 1:      # the quirk: a column of an ignoring frame still has a gradient when another frame keeps the point
        part = np.nonzero((lab == -1).any(axis=1) & (lab >= 0).any(axis=1))[0]
        assert len(part) > 5 and all(grad[n].reshape(S, C)[lab[n] == -1].all() for n in part)
    # margins: only the origin point is exempt
    mg = mf.margins_mf(pts, gt, loc, rot, mf.EXTRA)
    mg[origin] = np.inf
    assert mg.min() >= 1e-4


def test_union_boxes_restatement_and_the_unused_rotations(fx):
    gt, loc = fx["enl_gt"], fx["enl_loc"]
    e = mf.enlarged(gt, loc)
    assert np.abs(e - fx["enl64"]).max() <= 1e-9
    assert np.array_equal(e[..., [0, 1, 2, 5, 6, 7]], gt[..., [0, 1, 2, 5, 6, 7]].astype(np.float64))
    pad = gt[..., 3] == 0
    assert pad.any() and not e[pad].any()
    assert (e[~pad][:, 3] > gt[~pad][:, 3] + 0.1).any() and np.abs(fx["enl32"] - fx["enl64"]).max() <= 1e-4
    assert mf.enlarged(gt[:, :0], loc[:, :0]).shape == (3, 0, 8)
    still = np.repeat(gt[:, :, None, 0:3], 3, axis=2)      # a gt that does not move keeps its size
    assert np.abs(mf.enlarged(gt, still) - gt).max() <= 1e-5


def test_supported_predicate_at_each_bound():
    ok = dict(n=1000, batch=4, m=10, stack_frame_size=3, num_class=1)
    assert point_head_mf.supported(**ok)
    for k, good, bad in (("n", (0, 1 << 20), (-1, (1 << 20) + 1)), ("batch", (1, 64), (0, 65)), ("m", (0, 128), (-1, 129)),
                         ("stack_frame_size", (1, 8), (0, 9)), ("num_class", (1, 4), (0, 5))):
        for v in good:
            assert point_head_mf.supported(**dict(ok, **{k: v})), (k, v)
        for v in bad:
            assert not point_head_mf.supported(**dict(ok, **{k: v})), (k, v)
    assert (point_head_mf.MAX_FRAMES, point_head_mf.MAX_CLASS) == (8, 4)
    assert _lib.LIMITS["LIDAR_POINT_HEAD_MF_MAX_FRAMES"] == 8 and _lib.LIMITS["LIDAR_POINT_HEAD_MF_MAX_CLASS"] == 4
    assert point_head_mf.workspace_bytes(-1) == 0 and point_head_mf.workspace_bytes(0) > 0      # N = 0 still holds the count
    assert point_head_mf.workspace_bytes(257) > 0 and point_head_mf.workspace_bytes((1 << 20) + 1) == 0


def test_abi_refuses_bad_arguments_on_the_host():
    """every refusal happens before any launch or device access: dummy (never dereferenced) addresses, no GPU needed"""
    L = _lib.lib()
    a = torch.zeros(64)
    p, ew = _lib.ptr(a), _lib.host_f32(mf.EXTRA)

    def targets(n=10, b=2, m=5, s=3, nc=1, ew=ew, pts=p, g=p, lab=p):
        return L.lidar_point_targets_mf(pts, n, g, g, g, b, m, s, ew, nc, lab, None, None)
    for kw in (dict(n=-1), dict(n=(1 << 20) + 1), dict(b=0), dict(b=65), dict(m=-1), dict(m=129), dict(s=0), dict(s=9), dict(nc=0),
               dict(nc=5), dict(ew=None), dict(pts=None), dict(g=None), dict(lab=None)):
        assert targets(**kw) == -1, kw
    assert targets(n=0, pts=None, g=None, lab=None) == 0      # nothing to do

    def fwd(n=10, s=3, nc=1, x=p, lab=p, out=p, ws=p, nb=1 << 20):
        return L.lidar_point_loss_mf_forward(x, lab, n, s, nc, 1.0, out, ws, nb, None)

    def bwd(n=10, s=3, nc=1, x=p, lab=p, g=p, d=p, ws=p, nb=1 << 20):
        return L.lidar_point_loss_mf_backward(x, lab, n, s, nc, 1.0, g, d, ws, nb, None)
    for kw in (dict(n=-1), dict(n=(1 << 20) + 1), dict(s=0), dict(s=9), dict(nc=0), dict(nc=5), dict(x=None), dict(lab=None), dict(ws=None)):
        assert fwd(**kw) == -1 and bwd(**kw) == -1, kw
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(d=None) == -1
    assert fwd(nb=point_head_mf.workspace_bytes(10) - 1) == -3 and bwd(nb=point_head_mf.workspace_bytes(10) - 1) == -3
    assert bwd(n=0, x=None, lab=None, g=None, d=None, ws=None) == 0

    def enl(b=2, m=5, gd=8, s=3, g=p, loc=p, out=p):
        return L.lidar_multiframe_enlarged_boxes(g, loc, b, m, gd, s, out, None)
    for kw in (dict(b=0), dict(b=65), dict(m=-1), dict(m=129), dict(gd=7), dict(gd=9), dict(s=0), dict(s=9), dict(g=None),
               dict(loc=None), dict(out=None)):
        assert enl(**kw) == -1, kw
    assert enl(m=0, g=None, loc=None, out=None) == 0


def test_wrappers_refuse_wrong_dtypes_and_shapes():
    spec = point_head_mf.spec_from_cfg(mf.CASES["agnostic3"]["cfg"], 1)
    assert spec.box_coder is False and spec.cls_weight == 1.0      # the yaml's LOSS_REG: smooth-l1 is accepted: no box term
    pts, gt, loc, rot = torch.zeros(10, 4), torch.zeros(2, 5, 8), torch.zeros(2, 5, 3, 3), torch.zeros(2, 5, 3)
    E = _lib.LidarHipError
    for bad in (dict(points=torch.zeros(10, 3)), dict(points=pts.double()), dict(gt_boxes=torch.zeros(2, 5, 9)),
                dict(gt_boxes=torch.zeros(2, 5, 7)), dict(gt_boxes=gt.double()), dict(locations=torch.zeros(2, 5, 3)),
                dict(locations=torch.zeros(2, 4, 3, 3)), dict(locations=loc.double()), dict(rotations_y=torch.zeros(2, 5, 2)),
                dict(rotations_y=rot.double()), dict(locations=torch.zeros(2, 5, 9, 3), rotations_y=torch.zeros(2, 5, 9))):
        with pytest.raises(E):
            point_head_mf.assign_point_targets_mf(**dict(dict(points=pts, gt_boxes=gt, locations=loc, rotations_y=rot, spec=spec), **bad))
    with pytest.raises(E, match="CUDA"):      # all shapes right: the only thing missing is the device
        point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
    for g, l, r in ((torch.zeros(2, 5, 9), torch.zeros(2, 5, 3, 3), None), (torch.zeros(2, 5, 7), loc, None), (gt.double(), loc, None),
                    (gt, torch.zeros(2, 5, 3), None), (gt, loc, torch.zeros(2, 5, 2)), (gt, torch.zeros(2, 5, 9, 3), None)):
        with pytest.raises(E):
            point_head_mf.enlarged_gt_boxes(g, l, r)
    with pytest.raises(E, match="8 columns"):
        point_head_mf.enlarged_gt_boxes(torch.zeros(2, 5, 9), loc)
    with pytest.raises(E, match="CUDA"):
        point_head_mf.enlarged_gt_boxes(gt, loc, rot)
    lab = {"point_cls_labels_stacked": torch.zeros((10, 3), dtype=torch.int64)}
    for x, t, s in ((torch.zeros(10, 3), lab, 2), (torch.zeros(10, 2), lab, 3), (torch.zeros(10, 3).double(), lab, 3),
                    (torch.zeros(10, 3), {"point_cls_labels_stacked": torch.zeros((10, 3), dtype=torch.int32)}, 3),
                    (torch.zeros(10, 2), {"point_cls_labels": [torch.zeros(10, dtype=torch.int64)] * 2}, 3)):
        with pytest.raises(E):
            point_head_mf.point_head_loss_mf(x, t, spec, s)
    with pytest.raises(E, match="CUDA"):
        point_head_mf.point_head_loss_mf(torch.zeros(10, 3), lab, spec, 3)


def test_mirror_keeps_the_stack_frame_size_assertion(fx):
    head = make_head("agnostic3")
    assert head.cls_layers[-1].out_features == 3 and make_head("classes2").cls_layers[-1].out_features == 4
    pts, gt, loc, rot, _ = case_inputs(fx, "agnostic3")
    d = {"point_coords": torch.from_numpy(pts), "gt_boxes": torch.from_numpy(gt), "locations": torch.from_numpy(loc[:, :, :2]),
         "rotations_y": torch.from_numpy(rot[:, :, :2])}
    with pytest.raises(AssertionError, match="stack_frame_size=3"):
        head.assign_targets(d)
    with pytest.raises(AssertionError):
        make_head("agnostic3", stack_frame_size=3.0)
    assert dense_heads.PointHeadSimpleMultiFrame.__name__ in dense_heads.__all__


@pytest.mark.parametrize("name", list(mf.CASES))
def test_mirror_torch_formulation_on_cpu_tensors(fx, name):
    c = mf.CASES[name]
    S = c["frames"]
    head = make_head(name)
    pts, gt, loc, rot, x64 = case_inputs(fx, name)
    keep = [a.copy() for a in (pts, gt, loc, rot)]
    t = head.assign_targets({"point_coords": torch.from_numpy(pts), "gt_boxes": torch.from_numpy(gt), "locations": torch.from_numpy(loc),
                             "rotations_y": torch.from_numpy(rot)})
    assert isinstance(t, list) and len(t) == S and all(np.array_equal(a, b) for a, b in zip(keep, (pts, gt, loc, rot)))
    for s, d in enumerate(t):
        assert d["point_cls_labels"].dtype == torch.int64 and d["point_box_labels"] is None and d["point_part_labels"] is None
        assert np.array_equal(d["point_cls_labels"].numpy(), fx[f"{name}_labels"][:, s])
        assert np.array_equal(d["point_box_idx"].numpy(), fx[f"{name}_owner"][:, s])
    x = torch.from_numpy(x64).float().requires_grad_(True)
    head.forward_ret_dict = {"point_cls_preds": x, "point_cls_labels": [d["point_cls_labels"] for d in t]}
    loss, tb = head.get_loss()
    ref = json.loads(str(fx[f"{name}_tb64"]))
    assert list(tb) == list(ref) and tb["point_pos_num"] == ref["point_pos_num"]
    assert abs(tb["point_loss_cls"] - ref["point_loss_cls"]) <= 1e-5 * abs(ref["point_loss_cls"])
    loss.backward()
    e = fx[f"{name}_gcls64"]
    assert np.abs(x.grad.numpy() - e).max() <= 1e-5 * np.abs(e).max() and not x.grad.numpy()[e == 0].any()
    cls_loss, cls_tb = head.get_cls_layer_loss()
    assert list(cls_tb) == ["point_loss_cls", "point_pos_num"] and float(cls_loss) == tb["point_loss_cls"]


def test_mirror_forward_on_cpu_and_beyond_the_declared_support(fx):
    """forward() scores with the max over all frames and classes, reads the features the config names, and assigns targets in
    training; S = 9 and num_class = 5 lie beyond the kernels' support and take the torch formulation"""
    pts, gt, loc, rot, _ = case_inputs(fx, "agnostic3")
    head = make_head("agnostic3")
    feats = torch.randn(len(pts), 4)
    batch = {"point_features_before_fusion": feats, "point_features": feats + 100, "point_coords": torch.from_numpy(pts),
             "gt_boxes": torch.from_numpy(gt), "locations": torch.from_numpy(loc), "rotations_y": torch.from_numpy(rot)}
    head.train()
    out = head(batch)
    logits = head.forward_ret_dict["point_cls_preds"]
    assert logits.shape == (len(pts), 3) and torch.equal(logits, head.cls_layers(feats))
    assert torch.equal(out["point_cls_scores"], torch.sigmoid(logits).max(dim=-1).values)
    assert len(head.forward_ret_dict["point_cls_labels"]) == 3
    assert np.array_equal(torch.stack(head.forward_ret_dict["point_cls_labels"], 1).numpy(), fx["agnostic3_labels"])
    loss, tb = head.get_loss()
    assert tb["point_pos_num"] == float(fx["agnostic3_pos"]) and loss.requires_grad
    head.eval()
    head({"point_features_before_fusion": feats})
    assert "point_cls_labels" not in head.forward_ret_dict
    # beyond the support: 9 frames (the first three are the fixture's), 5 classes
    big = make_head("agnostic3", stack_frame_size=9, num_class=5)
    loc9, rot9 = np.concatenate([loc] * 3, axis=2), np.concatenate([rot] * 3, axis=2)
    t = big.assign_targets({"point_coords": torch.from_numpy(pts), "gt_boxes": torch.from_numpy(gt), "locations": torch.from_numpy(loc9),
                            "rotations_y": torch.from_numpy(rot9)})
    lab = np.stack([d["point_cls_labels"].numpy() for d in t], 1)
    e_lab, _ = mf.targets(pts, gt, loc9, rot9, mf.EXTRA, 5)
    assert np.array_equal(lab, e_lab) and not point_head_mf.supported(len(pts), 3, 6, 9, 5)
    x = torch.randn(len(pts), 45, requires_grad=True)
    big.forward_ret_dict = {"point_cls_preds": x, "point_cls_labels": [d["point_cls_labels"] for d in t]}
    loss, tb = big.get_loss()
    e_loss, e_pos, e_grad = mf.loss(x.detach().numpy(), e_lab, 5, 1.0)
    loss.backward()
    assert abs(float(loss) - e_loss) <= 1e-5 * e_loss and tb["point_pos_num"] == e_pos
    assert np.abs(x.grad.numpy() - e_grad).max() <= 1e-5 * np.abs(e_grad).max()


def test_sweep_inputs_are_clear_of_the_faces_and_decisive():
    seen = dict(pos=0, ignored=0, mixed_rows=0, pad_owner=0)
    cases = list(mf.sweep_cases())
    assert len({c[6] for c in cases}) == len(cases)
    for axis, values in ((0, mf.SWEEP_N), (1, mf.SWEEP_M), (2, mf.SWEEP_S), (3, mf.SWEEP_C), (4, mf.SWEEP_B), (5, mf.SWEEP_POS)):
        assert {c[axis] for c in cases} == set(values)
    for N, M, S, C, B, pos, seed in cases:
        pts, gt, loc, rot = mf.sweep_inputs(seed, N, M, S, C, B, pos)
        assert pts.shape == (N, 4) and gt.shape == (B, M, 8) and loc.shape == (B, M, S, 3) and rot.shape == (B, M, S)
        if N:
            assert mf.margins_mf(pts, gt, loc, rot, mf.EXTRA).min() >= 1e-4
        lab, own = mf.targets(pts, gt, loc, rot, mf.EXTRA, C)
        if pos == "none" or M == 0:
            assert not lab.any()
        elif pos == "all":
            assert (lab > 0).all()
        elif pos == "ignored":
            assert (lab == -1).all()
        elif M == 128 and N >= 255:
            frame = pts[:, 0].astype(int)
            seen["pos"] += int((lab > 0).sum())
            seen["ignored"] += int((lab == -1).sum())
            seen["mixed_rows"] += int(((lab == -1).any(axis=1) & (lab >= 0).any(axis=1)).sum())
            seen["pad_owner"] += int(((own >= 0) & (gt[frame[:, None], np.maximum(own, 0), 3] == 0)).sum())
            assert (own > 0).sum() >= 10 and (B == 1 or len(np.unique(frame)) > 1)
    assert seen["pos"] > 100 and seen["ignored"] > 20 and seen["mixed_rows"] > 5, seen
