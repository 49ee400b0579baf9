"""CPU-only checks of the second-stage target assignment (csrc/proposal_target.hip, lidardetection_amd/proposal_target.py, the
pcdet.models.roi_heads mirror): the numpy restatement of tests/_proposal_target_np.py reproduces every case of the reference's
fixture (which is what licenses it as the oracle of the GPU sweeps), the host-computed quotas, every refusal of the declared range
through the C ABI before any launch, and the options the mirror refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import _proposal_target_np as ptn
from lidardetection_amd import _lib, proposal_target
from lidardetection_amd.pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from lidardetection_amd.pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer
from lidardetection_amd.pcdet.utils.cfg import AttrDict
from oracle import c_oracle

INDEX_KEYS = ["sampled_inds", "roi_labels", "reg_valid_mask"]
BITWISE_KEYS = ["rois", "roi_scores", "gt_of_rois_src"]


def overlap(a, b):
    return c_oracle.pairwise(a, b, 0)


def close(got, exp, tol=1e-6):
    """|got - exp| <= tol * max(1, |exp|): a few float32 roundings at the value's own scale"""
    return bool(np.all(np.abs(got.astype(np.float64) - exp) <= tol * np.maximum(1.0, np.abs(exp))))


@pytest.mark.parametrize("name", ptn.CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    cfg, inp, exp = ptn.load_case(name)
    got = ptn.restate(cfg, inp["rois"], inp["roi_scores"], inp["roi_labels"], inp["gt_boxes"], inp["fg_keys"], inp["draws"],
                      gt_boxes_enlarged=inp.get("gt_boxes_enlarged"), overlap_fn=overlap)
    assert not got["frame_status"].any()
    for k in INDEX_KEYS + BITWISE_KEYS:
        assert np.array_equal(got[k], exp[k]), f"{name}: {k} differs in {int((got[k] != exp[k]).sum())} places"
    if cfg["CLS_SCORE_TYPE"] == "cls":
        assert got["rcnn_cls_labels"].dtype == exp["rcnn_cls_labels"].dtype == np.int64
        assert np.array_equal(got["rcnn_cls_labels"], exp["rcnn_cls_labels"])
    else:
        assert close(got["rcnn_cls_labels"], exp["rcnn_cls_labels"])
    assert close(got["max_overlaps"], exp["max_overlaps"]) and close(got["gt_iou_of_rois"], exp["gt_iou_of_rois"])
    assert close(got["gt_of_rois"], exp["gt_of_rois"]), np.abs(got["gt_of_rois"] - exp["gt_of_rois"]).max()


def test_fixture_holds_the_cases_it_claims():
    cfg, inp, exp = ptn.load_case("pv")
    ov = exp["max_overlaps"]
    fg = (ov >= 0.55).sum(1)
    hard = ((ov < 0.55) & (ov >= 0.1)).sum(1)
    easy = (ov < 0.1).sum(1)
    assert fg[0] > 64 and hard[0] and easy[0] and (fg[1], hard[1]) == (0, 0) and hard[2] + easy[2] == 0
    assert 0 < fg[3] < 64 and hard[3] and not easy[3]
    assert not inp["gt_boxes"][1].any()                                                   # a padding-only frame
    assert inp["gt_boxes"][0, 7].any() and ptn.kept_rows(inp["gt_boxes"][0]) == 7         # a real last row that sums to 0
    assert ((inp["rois"] == 0).all(-1) & (inp["roi_labels"] == 0)).any()                  # zero-padded rois with label 0
    assert (np.abs(inp["rois"][3, :, 6]) > np.pi).sum() >= 3                              # headings outside [-pi, pi]
    assert (exp["max_overlaps"] > 0.999).any()                                            # rois identical to a gt
    cfg, inp, _ = ptn.load_case("enlarged")
    trims = [(ptn.kept_rows(inp["gt_boxes"][b]), ptn.kept_rows(inp["gt_boxes_enlarged"][b])) for b in range(3)]
    assert any(a != b for a, b in trims) and any(a == b for a, b in trims), trims
    # no overlap within 1e-4 of a threshold in use: the condition for comparing index outputs exactly
    for name in ptn.CASES:
        cfg, _, exp = ptn.load_case(name)
        ov = exp["max_overlaps"]
        for key in ("REG_FG_THRESH", "CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO"):
            assert not ((np.abs(ov - np.float32(cfg[key])) < 1e-4) & (ov != 0) & (ov != 1)).any(), (name, key)


@pytest.mark.parametrize("ratio", [0.8, 0.3, 1 / 3, 0.55, 0.7, 0.0, 1.0])
def test_quotas_are_the_python_expressions(ratio):
    for P in (1, 7, 8, 128, 512):
        assert proposal_target.hard_quota_table(ratio, P) == [int(n * ratio) for n in range(P + 1)]
        assert proposal_target.fg_rois_per_image(ratio, P) == int(np.round(ratio * P))
    # a product that float32 rounds across an integer: 90 * 0.7 is 62.99999999999999 in double (int -> 62), 63.0 in float32
    assert proposal_target.hard_quota_table(0.7, 90)[90] == 62 and int(np.float32(0.7) * np.float32(90)) == 63


def _call(R=64, M=8, D=7, P=8, B=1, fg=4, quota=None, cls_type=1):
    q = (C.c_int * (max(P, 0) + 1))(*(quota if quota is not None else [int(n * 0.8) for n in range(max(P, 0) + 1)]))
    null = [None] * 12
    return _lib.lib().lidar_proposal_target(None, None, None, None, None, B, R, M, D, P, fg, q, 1, cls_type, 0.55, 0.75, 0.25, 0.1, 0.5,
                                            None, None, *null, None)


def test_launcher_refuses_the_outside_of_its_declared_range_before_any_launch():
    L = _lib.lib()
    assert L.lidar_proposal_target_supported(1, 1, 1, 7) == 1 and L.lidar_proposal_target_supported(1024, 512, 512, 16) == 1
    for bad in [dict(R=0), dict(R=1025), dict(M=0), dict(M=513), dict(D=6), dict(D=17), dict(P=0), dict(P=513)]:
        kw = dict(R=64, M=8, P=8, D=7)
        kw.update(bad)
        assert L.lidar_proposal_target_supported(kw["R"], kw["M"], kw["P"], kw["D"]) == 0, bad
        assert _call(**bad) == -1, bad                                     # LIDAR_ERR_ARG with null device pointers: nothing launched
    assert _call(B=-1) == -1 and _call(fg=9) == -1 and _call(fg=-1) == -1 and _call(cls_type=2) == -1
    assert _call(quota=[0, 2, 0, 0, 0, 0, 0, 0, 0]) == -1                  # hard_quota[n] must lie in [0, n]
    assert _call(B=0) == 0                                                 # an empty batch: nothing to do, nothing launched
    assert _call() == -1                                                   # in range, but the device pointers are null


def _host_inputs(B=2, R=16, M=4, D=7, P=8):
    return dict(rois=torch.zeros(B, R, D), roi_scores=torch.zeros(B, R), roi_labels=torch.zeros(B, R, dtype=torch.int64),
                gt_boxes=torch.zeros(B, M, D + 1), fg_keys=torch.zeros(B, R), draws=torch.zeros(B, P))


def _assign(t, **kw):
    args = dict(roi_per_image=8, fg_ratio=0.5, reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25, cls_bg_thresh_lo=0.1,
                hard_bg_ratio=0.8)
    args.update(kw)
    return proposal_target.assign(t["rois"], t["roi_scores"], t["roi_labels"], t["gt_boxes"], t["fg_keys"], t["draws"], **args)


def test_wrapper_checks_shapes_before_it_touches_the_device():
    t = _host_inputs()
    with pytest.raises(_lib.LidarHipError, match="gt_boxes_enlarged"):
        _assign(t, gt_boxes_enlarged=torch.zeros(2, 5, 8))
    with pytest.raises(_lib.LidarHipError, match="gt_boxes_enlarged"):
        _assign(t, gt_boxes_enlarged=torch.zeros(2, 4, 8, dtype=torch.float64))
    with pytest.raises(_lib.LidarHipError, match="gt_boxes must be"):
        _assign(dict(t, gt_boxes=torch.zeros(2, 4, 9)))
    with pytest.raises(_lib.LidarHipError, match="roi_labels"):
        _assign(dict(t, roi_labels=torch.zeros(2, 16, dtype=torch.int32)))
    with pytest.raises(_lib.LidarHipError, match="draws"):
        _assign(dict(t, draws=torch.zeros(2, 7)))
    with pytest.raises(_lib.LidarHipError, match="supported"):
        _assign(_host_inputs(R=1025))
    with pytest.raises(_lib.LidarHipError, match="supported"):
        _assign(_host_inputs(D=6))
    with pytest.raises(_lib.LidarHipError, match="CLS_SCORE_TYPE"):
        _assign(t, cls_score_type="raw_roi_iou")
    with pytest.raises(_lib.LidarHipError, match="CUDA"):                  # everything else in order: there is no CPU path
        _assign(t)


def test_mirror_refuses_tracking_targets_and_unknown_score_types():
    cfg = AttrDict(ptn.PV_RCNN_CFG)
    layer = ProposalTargetLayer(cfg)
    assert layer.roi_sampler_cfg is cfg
    head = RoIHeadTemplate(num_class=3, model_cfg=AttrDict(TARGET_CONFIG=cfg))
    assert isinstance(head.proposal_target_layer, ProposalTargetLayer) and head.num_class == 3
    with pytest.raises(NotImplementedError, match="REG_TRACKING_INFO"):
        ProposalTargetLayer(AttrDict(ptn.PV_RCNN_CFG, REG_TRACKING_INFO=True))
    with pytest.raises(NotImplementedError, match="CLS_SCORE_TYPE"):
        ProposalTargetLayer(AttrDict(ptn.PV_RCNN_CFG, CLS_SCORE_TYPE="raw_roi_iou"))
