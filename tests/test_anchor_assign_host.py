"""CPU checks of the anchor target assigner's host side (lidardetection_amd/anchor_assign.py and the pcdet mirror
dense_heads/target_assigner): class tables, output layout, unsupported options, the AnchorGenerator mirror.  No kernel runs."""
import numpy as np
import pytest
import torch

from lidardetection_amd import _lib, anchor_assign, pointpillar, synth
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
from lidardetection_amd.pcdet.utils.cfg import AttrDict

KITTI_GEN = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[h], align_center=False,
                  feature_map_stride=2, matched_threshold=m, unmatched_threshold=u)
             for n, (s, _, h), m, u in zip(["Car", "Pedestrian", "Cyclist"], pointpillar.KITTI_ANCHORS, [0.6, 0.5, 0.5],
                                           [0.45, 0.35, 0.35])]


class Coder:
    code_size, encode_angle_by_sincos = 7, False


def cfg(gen=KITTI_GEN, pos_fraction=-1.0, **extra):
    return AttrDict(ANCHOR_GENERATOR_CONFIG=gen, TARGET_ASSIGNER_CONFIG=AttrDict(
        NAME="AxisAlignedTargetAssigner", POS_FRACTION=pos_fraction, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False,
        MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"), **extra)


def test_class_table_wraps_id_zero_to_last_name():
    t = anchor_assign.class_table(["Car", "Pedestrian", "Cyclist"], ["Car", "Pedestrian", "Cyclist"])
    z = -anchor_assign.ID_MIN                 # entry of id 0
    assert len(t) == anchor_assign.NUM_IDS
    assert t[z:z + 5] == [2, 0, 1, 2, -1]     # id 0 -> class_names[-1]; ids past the names match nothing
    assert all(v == -1 for v in t[z + 4:])
    # numpy's wrap for negative ids: -1 -> class_names[-2], -2 -> class_names[-3], -3 -> out of range
    assert t[z - 3:z] == [-1, 0, 1]
    assert all(v == -1 for v in t[:z - 2])
    # a name without an anchor class, and anchor classes in another order
    assert anchor_assign.class_table(["Car", "Van", "Cyclist"], ["Cyclist", "Car"])[z:z + 4] == [0, 1, -1, 0]
    with pytest.raises(ValueError):
        anchor_assign.class_table(["Car"], ["Car", "Car"])


def test_seperate_multihead_key_as_the_reference_reads_it():
    heads = [dict(HEAD_CLS_NAME=["Car"]), dict(HEAD_CLS_NAME=["Pedestrian", "Cyclist"])]
    a = AxisAlignedTargetAssigner(cfg(USE_MULTIHEAD=True, SEPERATE_MULTIHEAD=True, RPN_HEAD_CFGS=heads),
                                  ["Car", "Pedestrian", "Cyclist"], Coder())
    assert a.remap == [1, 1, 2]
    # the configs' own spelling is not read by the reference: no remapping
    b = AxisAlignedTargetAssigner(cfg(USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True, RPN_HEAD_CFGS=heads),
                                  ["Car", "Pedestrian", "Cyclist"], Coder())
    assert b.remap == [0, 0, 0]
    # single head: the remapping lives on the multihead path only
    c = AxisAlignedTargetAssigner(cfg(SEPERATE_MULTIHEAD=True, RPN_HEAD_CFGS=heads), ["Car", "Pedestrian", "Cyclist"], Coder())
    assert c.remap == [0, 0, 0]
    assert a.class_of_id[-anchor_assign.ID_MIN:][:4] == [2, 0, 1, 2]


def _layout_reference(shapes, multihead):
    """output position of every (class, anchor) through the reference's own reshapes (axis_aligned_target_assigner.py:92-115),
    with anchor ids in place of targets"""
    ids, base = [], 0
    for s in shapes:
        n = int(np.prod(s[:-1]))
        ids.append(torch.arange(base, base + n))
        base += n
    if multihead:
        return torch.cat(ids)
    fmap = shapes[0][:3]
    return torch.cat([t.view(*fmap, -1) for t in ids], dim=-1).view(-1)


@pytest.mark.parametrize("multihead", [False, True])
def test_output_index_mapping(multihead):
    shapes = [(1, 5, 4, 1, 2, 7), (1, 5, 4, 2, 2, 7), (1, 5, 4, 1, 1, 7)] if not multihead else \
        [(1, 5, 4, 1, 2, 9), (1, 3, 2, 1, 2, 9), (1, 5, 4, 1, 1, 9)]
    per_loc, out_off, a_total = anchor_assign.output_layout(shapes, multihead)
    ref = _layout_reference(shapes, multihead)
    got = torch.empty_like(ref)
    base = 0
    for k, s in enumerate(shapes):
        n = int(np.prod(s[:-1]))
        i = torch.arange(n)
        got[(i // per_loc[k]) * a_total + out_off[k] + i % per_loc[k]] = torch.arange(base, base + n)
        base += n
    assert torch.equal(got, ref)
    if not multihead:
        assert (per_loc, out_off, a_total) == ([2, 4, 1], [0, 2, 6], 7)
        with pytest.raises(ValueError):
            anchor_assign.output_layout([(1, 5, 4, 1, 2, 7), (1, 4, 4, 1, 2, 7)], False)


def test_unsupported_options_raise():
    with pytest.raises(NotImplementedError, match="POS_FRACTION"):
        AxisAlignedTargetAssigner(cfg(pos_fraction=0.25), ["Car", "Pedestrian", "Cyclist"], Coder())
    with pytest.raises(NotImplementedError, match="match_height"):
        AxisAlignedTargetAssigner(cfg(), ["Car", "Pedestrian", "Cyclist"], Coder(), match_height=True)


def test_code_size_rule():
    assert anchor_assign.code_size_of(7, 7, False) == 7
    assert anchor_assign.code_size_of(10, 9, True) == 10      # NuScenes: 9-column gts, anchors padded to code_size 10
    assert anchor_assign.code_size_of(7, 9, False) == 7       # gt extras without anchor extras are dropped (zip)


def test_no_cpu_fallback():
    a = AxisAlignedTargetAssigner(cfg(), ["Car", "Pedestrian", "Cyclist"], Coder())
    anchors, _ = AnchorGenerator(synth.PP_RANGE, KITTI_GEN).generate_anchors([[8, 6]] * 3, device="cpu")
    with pytest.raises(_lib.LidarHipError):
        a.assign_targets(anchors, torch.zeros(1, 2, 8))


def test_workspace_query_is_pure_host():
    L = _lib.lib()
    assert L.lidar_anchor_assign_workspace_bytes(16, 60, 3) >= 16 * 60 * 32
    assert L.lidar_anchor_assign_workspace_bytes(16, 60, 17) == 0


def test_anchor_generator_matches_pointpillar_anchors():
    gen = AnchorGenerator(synth.PP_RANGE, KITTI_GEN)
    anchors, per_loc = gen.generate_anchors([[216, 248]] * 3, device="cpu")
    assert per_loc == [2, 2, 2]
    assert [tuple(a.shape) for a in anchors] == [(1, 248, 216, 1, 2, 7)] * 3
    flat = torch.cat(anchors, dim=-3).view(-1, 7)      # head order [y, x, class, rot]
    assert torch.equal(flat, pointpillar.generate_anchors(synth.PP_RANGE, (248, 216), "cpu"))
