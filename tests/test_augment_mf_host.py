"""CPU-only checks of the multi-frame poses through the train-time augmentation (lidar_augment_mf, lidardetection_amd/augment.py): the
numpy restatement of the pose path (tests/_augment_mf_np.py) against the reference's own output (tests/golden/augment_mf_ref.npz),
its agreement with the plain restatement on everything that is not a pose, the declared limits, and every refusal of the C ABI and the
wrapper that needs no device.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import _augment_mf_np as amf
import _augment_np as anp
from lidardetection_amd import _lib, augment


@pytest.mark.parametrize("name", amf.CASES)
def test_numpy_restatement_reproduces_the_reference(name):
    cfg, inp, exp, _ = amf.load_contract(name)
    out = amf.augment(inp, cfg)
    for k in ("point_offsets", "gt_counts", "sample_valid"):
        assert np.array_equal(out[k], exp[k]), k
    assert anp.close(out["points"], exp["points"]) and anp.close(out["gt_boxes"], exp["gt_boxes"])
    assert np.array_equal(out["gt_boxes"][..., 7], exp["gt_boxes"][..., 7])          # box row order: the class ids line up
    assert np.array_equal(out["points"][:, 3:], exp["points"][:, 3:])
    S = cfg["stack_frames"]
    assert out["locations"].shape == exp["locations"].shape == (*exp["gt_boxes"].shape[:2], S, 3)
    print(name, "max |d locations|", np.abs(out["locations"] - exp["locations"]).max(), "max |d rotations_y|",
          np.abs(out["rotations_y"] - exp["rotations_y"]).max())
    assert amf.pose_close(out, exp)
    for b, n in enumerate(exp["gt_counts"]):                                          # zero rows past the count, in both files
        assert not out["locations"][b, n:].any() and not out["rotations_y"][b, n:].any()
        assert not exp["locations"][b, n:].any() and not exp["rotations_y"][b, n:].any()


def test_golden_file_holds_the_situations_it_claims():
    frames, unfolded = {"yaml3": 3, "plane3": 3, "single": 1, "stack8": 8}, []
    for name in amf.CASES:
        cfg, inp, exp, _ = amf.load_contract(name)
        kinds = cfg["frames"]
        assert cfg["stack_frames"] == frames[name] == inp["locations"].shape[2] == inp["db_locations"].shape[1]
        assert np.all(inp["gt_boxes"][..., 7][inp["gt_boxes"][..., 3] > 0] >= 1)      # trained classes only
        e, k = kinds.index("empty"), kinds.index("blocked")
        assert inp["gt_counts"][e] == 0 and exp["sample_valid"][e].sum() > 0
        assert (inp["cand"][k] >= 0).sum() > 0 and exp["sample_valid"][k].sum() == 0
        assert cfg["stats"]["frames_dropping_both"] > 0 and cfg["stats"]["carved"] > 0
        assert inp["gt_boxes"].shape[1] <= 8 and inp["cand"].shape[1] * inp["cand"].shape[2] <= 30 and len(kinds) <= 4
        assert np.diff(inp["point_offsets"]).max() <= 1200 and np.diff(inp["db_offsets"]).max() <= 48
        unfolded.append(float(np.abs(exp["rotations_y"]).max()))
    assert max(unfolded) > np.pi                                                      # a rotations_y past the fold limit_period would apply
    c3, c1 = amf.load_contract("yaml3"), amf.load_contract("plane3")
    assert c3[1]["points"].shape[1] == 5 and c3[0]["flip"] == ["x"]
    assert c1[0]["plane"] and "sample_rot" in c1[1] and c1[0]["flip"] == ["x", "y"] and c1[1]["flip_y"].any() and c1[1]["flip_x"].any()


@pytest.mark.parametrize("name", amf.CASES)
def test_poses_change_nothing_else(name):
    cfg, inp, _, _ = amf.load_contract(name)
    with_p, without = amf.augment(inp, cfg), anp.augment(amf.without_poses(inp), cfg)
    for k in ("points", "point_offsets", "gt_boxes", "gt_counts", "sample_valid"):
        assert np.array_equal(with_p[k], without[k]), k


def test_class_id_0_rows_leave_the_poses_as_they_leave_the_boxes():
    inp, cfg = anp.synth_inputs(11, [300, 200], S=4, n_db=30)
    inp = amf.add_poses(inp, 2)
    assert amf.borderline_clear(inp, cfg)
    out = amf.augment(inp, cfg)
    n0 = int(inp["gt_counts"][0])
    trained = np.nonzero(inp["gt_boxes"][0, :n0, 7] > 0)[0]
    assert 0 < len(trained) < n0
    ident = dict(inp, flip_x=np.zeros(2, np.int32), flip_y=np.zeros(2, np.int32), rot=np.zeros(2, np.float32))
    cfg0 = dict(cfg, apply_scale=False, remove_outside_boxes=False)
    still = amf.augment(ident, cfg0)
    assert np.array_equal(still["locations"][0, :len(trained)], inp["locations"][0, trained])
    assert np.array_equal(still["rotations_y"][0, :len(trained)], inp["rotations_y"][0, trained])
    assert still["gt_counts"][0] == len(trained) + still["sample_valid"][0].sum()
    for b, n in enumerate(out["gt_counts"]):
        assert out["locations"][b, :n].any(axis=(1, 2)).all() and not out["locations"][b, n:].any()


def test_supported_limits():
    assert _lib.LIMITS["LIDAR_AUGMENT_MF_MAX_FRAMES"] == 8 == augment.MAX_FRAMES
    ok = _lib.lib().lidar_augment_mf_supported
    assert ok(4, 8, 3, 15, 1) and ok(4, 8, 3, 15, 8) and ok(5, 8, 2, 12, 3)
    assert not ok(4, 8, 3, 15, 0) and not ok(4, 8, 3, 15, 9) and not ok(4, 8, 3, 15, -1)
    assert not ok(2, 8, 3, 15, 3) and not ok(4, 8, 9, 15, 3) and not ok(4, 449, 1, 64, 3)      # what lidar_augment_supported refuses


def _abi(L, S=3, B=0, M=8, C=4):
    three, six = _lib.host_f32([0, 0, 0]), _lib.host_f32(anp.KITTI_RANGE)
    return L.lidar_augment_mf(None, None, 0, C, None, None, B, M, None, None, None, None, 0, 0, None, 3, 15, None, None, None, None, None,
                              None, None, three, None, six, 1, 1, 0, 0, None, None, None, None, S, None, None, None, None, None, None,
                              None, None, 0, None)


def test_c_abi_refusals_come_before_any_launch():
    L = _lib.lib()
    assert _abi(L) == 0 and _abi(L, S=1) == 0 and _abi(L, S=8) == 0            # B = 0 launches nothing
    assert _abi(L, S=0) == -1 and _abi(L, S=9) == -1 and _abi(L, C=9) == -1 and _abi(L, M=468) == -1
    assert _abi(L, B=2) == -1                                                   # null pointers with work to do


def _db(S=None, n=2, **kw):
    pose = {} if S is None else dict(locations=np.zeros((n, S, 3), np.float32), rotations_y=np.zeros((n, S), np.float32))
    pose.update(kw)
    return augment.GtDatabase(np.zeros((6, 4), np.float32), [0, 2, 6], np.ones((2, 7), np.float32), [1, 2], device="cpu", **pose)


def test_database_refusals():
    assert _db().S == 0 and _db().locations is None
    db = _db(3)
    assert db.S == 3 and tuple(db.locations.shape) == (2, 3, 3) and tuple(db.rotations_y.shape) == (2, 3) and db.locations.dtype == torch.float32
    for bad in (dict(locations=np.zeros((2, 3, 3))), dict(rotations_y=np.zeros((2, 3))),                    # one without the other
                dict(locations=np.zeros((2, 3, 3)), rotations_y=np.zeros((2, 2))),                          # S differs
                dict(locations=np.zeros((3, 3, 3)), rotations_y=np.zeros((3, 3))),                          # not n_obj rows
                dict(locations=np.zeros((2, 3, 2)), rotations_y=np.zeros((2, 3))),
                dict(locations=np.zeros((2, 9, 3)), rotations_y=np.zeros((2, 9))),                          # S = 9
                dict(locations=np.zeros((2, 0, 3)), rotations_y=np.zeros((2, 0)))):
        with pytest.raises(_lib.LidarHipError):
            _db(**bad)
            pytest.fail(str({k: v.shape for k, v in bad.items()}))


def test_wrapper_refusals():
    pts, offs = torch.zeros((10, 4)), torch.tensor([0, 10, 10], dtype=torch.int32)
    gt, cnt = torch.zeros((2, 8, 8)), torch.zeros(2, dtype=torch.int32)
    cand = np.full((2, 3, 15), -1, np.int32)
    kw = dict(flip_x=np.zeros(2), flip_y=np.zeros(2), rot=np.zeros(2), scale=np.ones(2))
    loc, ry = torch.zeros((2, 8, 3, 3)), torch.zeros((2, 8, 3))
    aug3, aug0, aug2 = (augment.TrainAugmentor(_db(S), 3, anp.KITTI_RANGE) for S in (3, None, 2))
    bad = [
        (aug3, dict(locations=loc), "one of them is missing"), (aug3, dict(rotations_y=ry), "one of them is missing"),
        (aug0, dict(locations=loc, rotations_y=ry), r"\(2, 8, 3, 3\).*database's locations are None"),      # no pose-carrying database
        (aug2, dict(locations=loc, rotations_y=ry), r"\(2, 8, 3, 3\).*\(2, 2, 3\)"),                         # another S
        (aug3, dict(locations=loc, rotations_y=ry[:, :, :2]), r"\(2, 8, 2\)"),
        (aug3, dict(locations=loc[:, :7], rotations_y=ry[:, :7]), r"\(2, 7, 3, 3\)"),
        (aug3, dict(locations=loc.double(), rotations_y=ry), "float64"),
        (aug3, dict(locations=loc[..., :2], rotations_y=ry), r"\(2, 8, 3, 2\)"),
    ]
    for aug, pose, msg in bad:
        with pytest.raises(_lib.LidarHipError, match=msg):
            aug(pts, offs, gt, cnt, cand, **kw, **pose)
    with pytest.raises(_lib.LidarHipError, match="CUDA"):                 # consistent poses: only the device is missing
        aug3(pts, offs, gt, cnt, cand, **kw, locations=loc, rotations_y=ry)
    with pytest.raises(_lib.LidarHipError, match="CUDA"):                 # and without poses the call is as before
        aug3(pts, offs, gt, cnt, cand, **kw)
