"""Host side of the fused anchor-head loss (lidardetection_amd/anchor_loss.py): the loss spec read from the reference's configs, the
per-head column tables, the refusals, the workspace query, and `restated_loss` (tests/_anchor_loss_torch.py) — a torch restatement
of the reference's RPN loss written for these tests — checked against the reference's own fp64 losses and autograd gradients (tests/golden/anchor_loss_ref.npz,
written by tests/golden/make_loss_golden.py).  The GPU tests trust the restatement at sizes the fixture cannot hold only because
it reproduces the fixture here."""
import numpy as np
import pytest
import torch

from lidardetection_amd import _lib, anchor_loss
from lidardetection_amd.pcdet.utils.cfg import AttrDict

from _anchor_loss_torch import CASES, direction_bins, load_case, per_head, restated_loss

# inline copies of the DENSE_HEAD loss settings of tools/cfgs/kitti_models/pointpillar.yaml,
# tools/cfgs/nuscenes_models/cbgs_second_multihead.yaml and tools/cfgs/kitti_models/second_multihead.yaml
POINTPILLAR = AttrDict(USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                       LOSS_CONFIG=AttrDict(LOSS_WEIGHTS={"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2,
                                                          "code_weights": [1.0] * 7}))
CBGS_SECOND_MULTIHEAD = AttrDict(DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2, USE_MULTIHEAD=True,
                                 SEPARATE_MULTIHEAD=True,
                                 LOSS_CONFIG=AttrDict(REG_LOSS_TYPE="WeightedL1Loss", LOSS_WEIGHTS={
                                     "pos_cls_weight": 1.0, "neg_cls_weight": 2.0, "cls_weight": 1.0, "loc_weight": 0.25,
                                     "dir_weight": 0.2, "code_weights": [1.0] * 8 + [0.2, 0.2]}))
SECOND_MULTIHEAD = AttrDict(USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                            USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True,
                            LOSS_CONFIG=AttrDict(LOSS_WEIGHTS={"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2,
                                                               "code_weights": [1.0] * 7}))


# ------------------------------------------------------------------------------------------------ tests
def test_spec_pointpillar():
    s = anchor_loss.spec_from_cfg(POINTPILLAR, 3)
    assert (s.multihead, s.separate, s.head_classes, s.head_class_offsets) == (False, False, (3,), (0,))
    assert (s.cls_weight, s.loc_weight, s.dir_weight, s.pos_cls_weight, s.neg_cls_weight) == (1.0, 2.0, 0.2, 1.0, 1.0)
    assert s.reg_loss == "WeightedSmoothL1Loss" and s.use_dir and s.num_dir_bins == 2 and s.dir_offset == 0.78539
    assert s.code_weights == (1.0,) * 7


def test_spec_cbgs_second_multihead():
    s = anchor_loss.spec_from_cfg(CBGS_SECOND_MULTIHEAD, 10, [1, 2, 2, 1, 2, 2])
    assert s.multihead and s.separate and not s.use_dir
    assert s.head_classes == (1, 2, 2, 1, 2, 2) and s.head_class_offsets == (0, 1, 3, 5, 6, 8)
    assert (s.pos_cls_weight, s.neg_cls_weight, s.loc_weight, s.dir_weight) == (1.0, 2.0, 0.25, 0.0)
    assert s.reg_loss == "WeightedL1Loss" and s.code_weights[8:] == (0.2, 0.2) and len(s.code_weights) == 10


def test_spec_second_multihead_and_unseparated():
    s = anchor_loss.spec_from_cfg(SECOND_MULTIHEAD, 3, [1, 1, 1])
    assert s.head_classes == (1, 1, 1) and s.head_class_offsets == (0, 1, 2) and s.use_dir
    assert (s.pos_cls_weight, s.neg_cls_weight) == (1.0, 1.0)      # no pos_cls_weight in LOSS_WEIGHTS
    cfg = AttrDict(SECOND_MULTIHEAD)
    cfg.pop("SEPARATE_MULTIHEAD")
    s = anchor_loss.spec_from_cfg(cfg, 3, [3, 3, 3])
    assert not s.separate and s.head_classes == (3, 3, 3) and s.head_class_offsets == (0, 0, 0)
    cfg = AttrDict(SECOND_MULTIHEAD, SEPERATE_MULTIHEAD=True)      # the assigner's misspelled key is not the loss's
    cfg.pop("SEPARATE_MULTIHEAD")
    assert not anchor_loss.spec_from_cfg(cfg, 3, [3, 3, 3]).separate


def test_spec_refusals():
    bad = AttrDict(POINTPILLAR, LOSS_CONFIG=AttrDict(REG_LOSS_TYPE="WeightedBalancedL1", LOSS_WEIGHTS=POINTPILLAR.LOSS_CONFIG.LOSS_WEIGHTS))
    with pytest.raises(NotImplementedError):
        anchor_loss.spec_from_cfg(bad, 3)
    with pytest.raises(NotImplementedError):
        anchor_loss.spec_from_cfg(SECOND_MULTIHEAD, 17, [1] * 17)
    long_code = AttrDict(POINTPILLAR, LOSS_CONFIG=AttrDict(LOSS_WEIGHTS=dict(POINTPILLAR.LOSS_CONFIG.LOSS_WEIGHTS,
                                                                            code_weights=[1.0] * 17)))
    with pytest.raises(NotImplementedError):
        anchor_loss.spec_from_cfg(long_code, 3)
    with pytest.raises(NotImplementedError):
        anchor_loss.spec_from_cfg(AttrDict(POINTPILLAR, NUM_DIR_BINS=9), 3)
    with pytest.raises(ValueError):
        anchor_loss.spec_from_cfg(SECOND_MULTIHEAD, 2, [1, 1, 1])


def test_non_fp32_and_host_tensors_refused():
    spec = anchor_loss.spec_from_cfg(POINTPILLAR, 3)
    labels = torch.zeros(1, 6, dtype=torch.int32)
    targets = torch.zeros(1, 6, 7)
    with pytest.raises(_lib.LidarHipError, match="float32"):
        anchor_loss.anchor_head_loss(torch.zeros(1, 6, 3, dtype=torch.float64), torch.zeros(1, 6, 7), None, labels, targets, None,
                                     spec)
    with pytest.raises(_lib.LidarHipError):   # no CPU path
        anchor_loss.anchor_head_loss(torch.zeros(1, 6, 3), torch.zeros(1, 6, 7), None, labels, targets, None, spec)


def test_workspace_query_is_pure_host():
    assert anchor_loss.workspace_bytes(16, [321408]) >= 16 * (321408 // 256) * 16
    assert anchor_loss.workspace_bytes(4, [32768, 65536, 65536, 32768, 65536, 65536]) > 0
    L = _lib.lib()
    assert anchor_loss.workspace_bytes(0, [10]) == 0
    assert anchor_loss.workspace_bytes(1, [0]) == 0
    assert anchor_loss.workspace_bytes(1, [1] * 17) == 0
    assert L.lidar_anchor_loss_forward(None, None, None, None, None, None, 0, None, None, None, 0, 0, 0, 0, 0, 0, None, None, 0,
                                       None, None, 0, None) == -1


@pytest.mark.parametrize("name", CASES)
def test_fixture_tables(name):
    meta, preds, _, arr = load_case(name)
    spec, cls, box, _ = per_head(meta, preds, meta["batch"])
    assert sum(x.shape[1] for x in cls) == arr["labels"].shape[1] == arr["anchors"].shape[0]
    assert [x.shape[1] for x in box] == [x.shape[1] for x in cls]
    if spec.separate:
        assert sum(spec.head_classes) == spec.num_class
        assert list(spec.head_class_offsets) == list(np.cumsum([0, *spec.head_classes[:-1]]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    meta, preds, grads, arr = load_case(name)
    B = meta["batch"]
    spec, cls, box, dirs = per_head(meta, preds, B)
    leaves = [x.double().requires_grad_() for x in cls + box + dirs]
    H = len(cls)
    losses = restated_loss(leaves[:H], leaves[H:2 * H], leaves[2 * H:], arr["labels"], arr["targets"], arr["anchors"], spec)
    got = torch.stack([x.detach() for x in losses])
    assert torch.allclose(got, arr["loss64"], rtol=1e-12, atol=1e-12), (got, arr["loss64"])
    sum(losses).backward()
    want = grads["cls"] + grads["box"] + grads["dir"]
    zero = grads["zero"]["cls"] + grads["zero"]["box"] + grads["zero"]["dir"]
    for leaf, g, z in zip(leaves, want, zero):
        g = g.double().reshape(leaf.shape)
        scale = g.abs().max().clamp(min=1e-30)
        assert ((leaf.grad - g).abs() / scale).max() < 1e-6
        assert torch.equal(leaf.grad == 0, z.reshape(leaf.shape))
    # fp32 restatement against the reference's fp32 run
    got32 = torch.stack(restated_loss(cls, box, dirs, arr["labels"], arr["targets"], arr["anchors"], spec)).double()
    assert torch.allclose(got32, arr["loss32"], rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["kitti", "kitti_multi"])
def test_mirror_static_helpers(name):
    """AnchorHeadTemplate.get_direction_target / add_sin_difference (pure torch) on the fixture's targets and anchors"""
    from lidardetection_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
    meta, _, _, arr = load_case(name)
    B = meta["batch"]
    targets, anchors = arr["targets"], arr["anchors"]
    rep = anchors.unsqueeze(0).repeat(B, 1, 1)          # the reference passes the anchors repeated per frame
    bins = direction_bins(targets, anchors, 0.78539, 2)
    one_hot = AnchorHeadTemplate.get_direction_target(rep, targets, dir_offset=0.78539, num_bins=2)
    assert one_hot.dtype == anchors.dtype and one_hot.shape == (B, anchors.shape[0], 2)
    assert torch.equal(one_hot.argmax(-1), bins) and torch.equal(one_hot.sum(-1), torch.ones_like(one_hot[..., 0]))
    assert torch.equal(AnchorHeadTemplate.get_direction_target(rep, targets, one_hot=False, dir_offset=0.78539, num_bins=2), bins)
    pred = torch.randn(B, anchors.shape[0], targets.shape[-1], dtype=torch.float64, requires_grad=True)
    p2, t2 = AnchorHeadTemplate.add_sin_difference(pred, targets.double())
    keep = [q for q in range(targets.shape[-1]) if q != 6]
    assert torch.equal(p2[..., keep], pred[..., keep]) and torch.equal(t2[..., keep], targets.double()[..., keep])
    assert torch.allclose(p2[..., 6] - t2[..., 6], torch.sin(pred[..., 6] - targets.double()[..., 6]), atol=1e-12)
    p2.sum().backward()
    assert torch.allclose(pred.grad[..., 6], torch.cos(pred[..., 6]) * torch.cos(targets.double()[..., 6]))
    with pytest.raises(ValueError):
        AnchorHeadTemplate.add_sin_difference(pred, targets.double(), dim=-1)
