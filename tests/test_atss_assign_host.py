"""ATSS anchor target assignment, host side (lidardetection_amd/atss_assign.py, csrc/atss_assign.hip's pure-host entry points, the
pcdet mirror): the numpy restatement of tests/_atss_np.py reproduces every case of the reference's own ATSSTargetAssigner
(tests/golden/atss_assign_ref.npz, written by tests/golden/make_atss_golden.py) from the IoU matrices the reference saw, which
pins its tie rules where the fixture has such cases (two gts forcing anchor 0: the later one wins; a gt that overlaps nothing:
anchor 0); the rules are then shown on their own on un-jittered grids.  No GPU is needed."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import _atss_np as atn
from lidardetection_amd import _lib, atss_assign
from lidardetection_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
from lidardetection_amd.pcdet.models.dense_heads.target_assigner import atss_target_assigner
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.atss_target_assigner import ATSSTargetAssigner
from lidardetection_amd.pcdet.utils.cfg import AttrDict

CASES, load_case = atn.CASES, atn.load_case


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    meta, _, flat, gt, ious, (labels, targets, weights) = load_case(name)
    got = atn.assign(flat, gt, meta["topk"], meta["code_size"], meta["encode_angle_by_sincos"], lambda b, k, a, g: ious[(b, k)])
    assert np.array_equal(got[0], labels.astype(np.int32)) and np.array_equal(labels, labels.astype(np.int32))
    assert np.array_equal(got[2], weights)
    assert np.abs(got[1] - targets).max() <= 1e-6
    assert (labels > 0).sum() > 0


def test_fixture_holds_the_tie_cases():
    """kitti frame 0: rows 3 (all zero, class 0) and 4 (outside the range, class 2) both force anchor 0 of every set; the
    reference labels it 2, so the later gt won.  Frame 1 is only padding; negative and zero class ids come through."""
    meta, _, flat, gt, ious, (labels, _, weights) = load_case("kitti")
    off = 0
    for k, a in enumerate(flat):
        assert ious[(0, k)][:, 3].max() == 0 and ious[(0, k)][:, 4].max() == 0
        assert labels[0, off] == 2 and weights[0, off] == 1
        off += a.shape[0]
    assert not labels[1].any() and not weights[1].any()
    assert (labels[0] == -1).any() and (gt[0, :, -1] == 0).sum() >= 2
    assert atn.trim_count(gt[0, :, :-1]) == 9 and gt[0, 9, 0] == 1.0     # the trailing [1, -1, 0, ...] row is trimmed


def _grid_anchors(cfg, pc_range, grid):
    sets, _ = AnchorGenerator(pc_range, cfg).generate_anchors([grid] * len(cfg), device="cpu")
    return [a.reshape(-1, a.shape[-1]).numpy() for a in sets]


def _host_iou(b, k, a, g):
    out = torch.zeros((a.shape[0], g.shape[0]), dtype=torch.float32)
    at, gt_ = torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(g))
    _lib.check(_lib.lib().lidar_boxes_iou_bev_cpu(_lib.ptr(at), a.shape[0], _lib.ptr(gt_), g.shape[0], _lib.ptr(out)), "iou")
    return out.numpy()


def test_tie_rules_on_unjittered_grid():
    cfg = [dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
                align_center=False, feature_map_stride=2)]
    (a,) = _grid_anchors(cfg, [0.0, -7.2, -3, 17.6, 7.2, 1], [12, 10])
    # top-k: both rotations of a location are equally far; the lower index goes first
    g = np.array([[a[100, 0], a[100, 1], a[100, 2], 3.9, 1.6, 1.56, 0.0]], np.float32)
    d = atn.distances(a, g)[:, 0]
    assert d[100] == d[101] == 0
    assert atn.topk_candidates(d, 1).tolist() == [100] and atn.topk_candidates(d, 3)[:2].tolist() == [100, 101]
    assert atn.topk_candidates(d, 3)[2] == min(i for i in range(len(a)) if i not in (100, 101) and d[i] == np.sort(d)[2])
    # two identical gts on one anchor: the anchor is positive for both with the same IoU -> the lowest gt would keep it, but both
    # also force it -> the highest gt wins; a third gt far outside forces anchor 0
    gt = np.zeros((1, 4, 8), np.float32)
    gt[0, 0] = [*a[100, :7], 1]
    gt[0, 1] = [*a[100, :7], 3]
    gt[0, 2] = [300.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 2]
    labels, targets, weights = atn.assign([a], gt, 9, 7, False, _host_iou)
    assert labels[0, 100] == 3 and labels[0, 0] == 2 and weights[0, 100] == 1
    assert np.abs(targets[0, 100]).max() == 0          # the gt is the anchor
    # per-anchor maximum over gts without a force: the positive candidates of two identical gts other than the forced anchor
    # (none here has a larger IoU than the anchor itself) stay with the lowest gt
    others = [i for i in np.nonzero(labels[0] > 0)[0] if i not in (0, 100)]
    assert all(labels[0, i] == 1 for i in others)


def test_supported_ranges():
    L = _lib.lib()

    def ok(counts=(240, 240), D=7, gt_cols=8, code=7, sincos=0, topk=9, M=12, mh=0):
        arr = (C.c_longlong * max(len(counts), 1))(*counts)
        return L.lidar_atss_assign_supported(arr, len(counts), D, gt_cols, code, sincos, topk, M, mh)

    assert ok() == 1 and ok(mh=1) == 1
    assert ok(counts=(240,) * 16) == 1 and ok(counts=(240,) * 17) == 0 and ok(counts=()) == 0
    assert ok(D=6) == 0 and ok(D=9, gt_cols=10, code=9) == 1 and ok(D=9, gt_cols=10, code=10, sincos=1) == 1
    assert ok(D=16, gt_cols=17, code=16) == 1 and ok(D=17, gt_cols=18, code=17) == 0
    assert ok(code=8) == 0 and ok(code=8, sincos=1) == 1 and ok(sincos=2) == 0
    assert ok(topk=1) == 0 and ok(topk=2) == 1 and ok(topk=32) == 1 and ok(topk=33) == 0
    assert ok(counts=(9, 240)) == 1 and ok(counts=(8, 240)) == 0 and ok(counts=(2,), topk=2) == 1
    assert ok(M=0) == 0 and ok(M=1) == 1 and ok(M=256) == 1 and ok(M=257) == 0
    assert ok(mh=2) == 0 and ok(mh=-1) == 0
    assert atss_assign.supported([240], 7, 8, 7, False, 9, 12, False) and not atss_assign.supported([240], 7, 8, 7, False, 1, 12, False)


def test_workspace_bytes_monotone():
    base = dict(batch=2, max_gt=12, num_sets=3, topk=9)
    b0 = atss_assign.workspace_bytes(**base)
    assert b0 >= 2 * 3 * 12 * 10 * 12
    for key, hi in [("batch", 16), ("max_gt", 256), ("num_sets", 16), ("topk", 32)]:
        prev = 0
        for v in range(base[key] if key != "topk" else 2, hi + 1):
            cur = atss_assign.workspace_bytes(**{**base, key: v})
            assert cur >= prev > -1
            prev = cur
        assert prev > b0 or base[key] == hi
    assert atss_assign.workspace_bytes(2, 257, 3, 9) == 0 and atss_assign.workspace_bytes(2, 12, 3, 1) == 0


class _Coder:
    code_size, encode_angle_by_sincos = 7, False


def test_call_forms():
    """the class's own form (topk, box_coder, match_height) and the head's (use_multihead=, gt_boxes_enlarged=)"""
    a = ATSSTargetAssigner(9, _Coder(), match_height=True)
    assert (a.topk, a.match_height, a.use_multihead) == (9, True, False)
    b = ATSSTargetAssigner(topk=9, box_coder=_Coder(), use_multihead=True, match_height=False)
    assert b.use_multihead and not b.match_height
    with pytest.raises(ValueError):
        ATSSTargetAssigner(1, _Coder())
    gt = torch.zeros((1, 2, 8))
    with pytest.raises(NotImplementedError):
        b.assign_targets([torch.zeros((1, 2, 2, 1, 2, 7))], gt, gt_boxes_enlarged=gt)
    with pytest.raises(NotImplementedError):
        a.assign_targets(torch.zeros((1, 2, 2, 1, 2, 7)), gt, use_multihead=False, gt_boxes_enlarged=gt)
    # past the enlarged check the call reaches the device layer, which refuses host tensors: both call forms get that far
    for call in (lambda: a.assign_targets(torch.zeros((1, 4, 4, 1, 2, 7)), gt),
                 lambda: b.assign_targets([torch.zeros((1, 4, 4, 1, 2, 7))], gt, use_multihead=True, gt_boxes_enlarged=None)):
        with pytest.raises(_lib.LidarHipError, match="CUDA"):
            call()
    assert "TypeError" in atss_target_assigner.__doc__


def _head_stub(use_multihead=False):
    return types.SimpleNamespace(box_coder=_Coder(), use_multihead=use_multihead, model_cfg=None, class_names=["Car"])


def test_get_target_assigner():
    t = AnchorHeadTemplate.get_target_assigner(_head_stub(True), AttrDict(NAME="ATSS", TOPK=9, MATCH_HEIGHT=False))
    assert isinstance(t, ATSSTargetAssigner) and t.topk == 9 and t.use_multihead and not t.match_height
    with pytest.raises(NotImplementedError):
        AnchorHeadTemplate.get_target_assigner(_head_stub(), AttrDict(NAME="SomethingElse", TOPK=9, MATCH_HEIGHT=False))
