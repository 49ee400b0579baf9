"""CPU-only checks of the train-time augmentation (lidardetection_amd/augment.py, csrc/augment.hip): the numpy restatement of the
contract (tests/_augment_np.py) against the reference's own output (tests/golden/augment_ref.npz), the host sampler against the
reference's recorded draws, the road-plane closed form, the PREPARE filters, and every refusal of lidar_augment_supported, the C ABI
and the wrapper.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import _augment_np as anp
from lidardetection_amd import _lib, augment


class ReplayRng:
    """hands out the reference's recorded permutations, in order"""
    def __init__(self, perms):
        self.perms = list(perms)

    def permutation(self, n):
        p = self.perms.pop(0)
        assert len(p) == n, "the sampler reshuffles a pool of another size than the reference did"
        return p


def _perms(z, name):
    flat, lens = z[f"{name}_rec_perms"], z[f"{name}_rec_perm_len"]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [flat[cuts[i]:cuts[i + 1]] for i in range(len(lens))]


def _db(inp, z, name, device="cpu"):
    return augment.GtDatabase(inp["db_points"], inp["db_offsets"], inp["db_boxes"], inp["db_cls"],
                              difficulty=z[f"{name}_rec_db_difficulty"], device=device)


@pytest.mark.parametrize("name", anp.CASES)
def test_numpy_restatement_reproduces_the_reference(name):
    cfg, inp, exp, _ = anp.load_contract(name)
    out = anp.augment(inp, cfg)
    for k in ("point_offsets", "gt_counts", "sample_valid"):
        assert np.array_equal(out[k], exp[k]), k
    assert anp.close(out["points"], exp["points"]) and anp.close(out["gt_boxes"], exp["gt_boxes"])
    assert np.array_equal(out["gt_boxes"][..., 7], exp["gt_boxes"][..., 7])          # box row order: the class ids line up
    assert np.array_equal(out["points"][:, 3:], exp["points"][:, 3:])                # kept-row order: the features are copied bits


def test_golden_file_holds_the_situations_it_claims():
    cfg, inp, exp, _ = anp.load_contract("kitti")
    assert cfg["stats"]["only_untrained"] > 0 and cfg["stats"]["only_each_other"] > 0 and cfg["stats"]["carved"] > 0
    assert inp["gt_counts"][1] == 0 and exp["sample_valid"][1].sum() > 0              # a frame with no annotations still gets samples
    assert (inp["cand"][2] >= 0).sum() > 0 and exp["sample_valid"][2].sum() == 0      # every candidate of frame 2 collides
    assert np.any(inp["gt_boxes"][0, :inp["gt_counts"][0], 7] == 0)                   # untrained rows
    assert anp.load_case("feat5")[1]["points"].shape[1] == 5
    assert anp.load_case("corners8")[0]["min_num_corners"] == 8
    for name in anp.CASES:
        c, i, e = anp.load_case(name)
        live = i["cand"] >= 0
        assert e["sample_valid"][live].min() == 0 and e["sample_valid"][live].max() == 1, name


@pytest.mark.parametrize("name", anp.CASES)
def test_db_sampler_replays_the_reference(name):
    cfg, inp, exp, z = anp.load_contract(name)
    db = _db(inp, z, name)
    sampler = augment.DbSampler(db, cfg["groups"], removed_difficulty=cfg["removed_difficulty"],
                                min_points={int(k): v for k, v in cfg["min_points"].items()}, limit_whole_scene=cfg["limit_whole_scene"])
    perms = _perms(z, name)
    counts = inp["gt_counts"]
    cuts = np.concatenate([[0], np.cumsum(counts)])
    classes = [z[f"{name}_rec_gt_classes"][cuts[b]:cuts[b + 1]] for b in range(len(counts))]
    rng = ReplayRng(perms)
    cand = sampler.sample(classes, rng)
    assert cand.dtype == np.int32 and np.array_equal(cand, inp["cand"])
    assert not rng.perms, "the reference reshuffled more often"
    if name == "kitti":                # 19 cars, 15 per frame: the pointer runs past the end and the pool is reshuffled
        assert len(perms) > len(cfg["groups"])
        assert (inp["cand"][1, 0] >= 0).sum() < 15


def test_road_plane_lidar_matches_put_boxes_on_road_planes():
    z = np.load(anp.GOLDEN)
    h = z["kitti_rec_heights"]            # frame, x, y, z, dz, mv_height of the reference
    assert len(h) > 20
    for row in h:
        b = int(row[0])
        q = augment.road_plane_lidar(z["kitti_rec_plane_abcd"][b], z["kitti_rec_V2C"][b], z["kitti_rec_R0"][b])
        mv = row[3] - row[4] / 2 - (q[:3] @ row[1:4] + q[3])
        assert abs(mv - row[5]) <= 1e-4 * max(1.0, abs(row[5]))


def test_prepare_filters_and_fakelidar():
    pts = np.zeros((10, 4), np.float32)
    offs = [0, 1, 3, 6, 10]
    boxes = np.array([[1, 2, 3, 1.6, 3.9, 1.5, 0.3]] * 4, np.float32)
    db = augment.GtDatabase(pts, offs, boxes, [1, 1, 2, 1], difficulty=[0, -1, 0, 2], device="cpu")
    assert db.indices_of_class(1).tolist() == [0, 1, 3]
    assert db.indices_of_class(1, removed_difficulty=[-1]).tolist() == [0, 3]
    assert db.indices_of_class(1, min_points=2).tolist() == [1, 3]
    assert db.indices_of_class(1, removed_difficulty=[-1, 2], min_points=1).tolist() == [0]
    assert db.indices_of_class(3).tolist() == []
    fake = augment.GtDatabase(pts, offs, boxes, [1, 1, 2, 1], fakelidar=True, device="cpu")
    got = fake.boxes.numpy()
    assert np.allclose(got[0], [1, 2, 3 + 0.75, 3.9, 1.6, 1.5, -(0.3 + np.pi / 2)], atol=1e-6)
    assert np.allclose(fake.points.numpy()[:, 2], -0.75)          # the object still lands on the unconverted (bottom) centre
    with pytest.raises(_lib.LidarHipError):
        augment.GtDatabase(pts, [0, 1, 3, 6, 9], boxes, [1, 1, 2, 1], device="cpu")
    with pytest.raises(_lib.LidarHipError):
        augment.GtDatabase(pts, offs, boxes, [1, 0, 2, 1], device="cpu")


def test_supported_limits():
    ok = _lib.lib().lidar_augment_supported
    assert ok(3, 8, 1, 0) and ok(8, 8, 8, 63) and ok(4, 512 - 8 * 64, 8, 64) and ok(4, 512, 1, 0) and ok(4, 0, 3, 15)
    assert not ok(2, 8, 3, 15) and not ok(9, 8, 3, 15)                     # 3 <= C <= 8
    assert not ok(4, 8, 0, 15) and not ok(4, 8, 9, 15)                     # 1 <= G <= 8
    assert not ok(4, 8, 3, -1) and not ok(4, 8, 3, 65)                     # 0 <= S <= 64
    assert not ok(4, 9, 8, 63) and not ok(4, 513, 1, 0) and ok(4, 448, 1, 64) and not ok(4, 449, 1, 64)      # M + G S <= 512
    assert not ok(4, -1, 3, 15)


def _abi(L, C=4, M=8, G=3, S=15, B=0, n_points=0, bound=0, cap=0, corners=1, rw=True, rng=True):
    three, six = _lib.host_f32([0, 0, 0]), _lib.host_f32(anp.KITTI_RANGE)
    return L.lidar_augment(None, None, n_points, C, None, None, B, M, None, None, None, None, 0, 0, None, G, S, None, None, None, None,
                           None, None, None, three if rw else None, None, six if rng else None, 1, corners, bound, cap, None, None,
                           None, None, None, None, 0, None)


def test_c_abi_refusals_come_before_any_launch():
    L = _lib.lib()
    assert _abi(L) == 0                                                     # B = 0 launches nothing
    assert _abi(L, cap=100, n_points=60, bound=40) == 0
    assert _abi(L, cap=99, n_points=60, bound=40) == -1                     # cap below the bound
    for bad in (dict(C=2), dict(C=9), dict(G=0), dict(G=9), dict(S=65), dict(S=-1), dict(M=468), dict(B=-1), dict(corners=9),
                dict(corners=-1), dict(rw=False), dict(rng=False), dict(n_points=-1), dict(bound=-1)):
        assert _abi(L, **bad) == -1, bad
    assert _abi(L, M=467) == 0
    assert _abi(L, B=2) == -1                                               # null pointers with work to do
    assert L.lidar_augment_workspace_bytes(0, 3, 15, 1000) == 0
    small, big = L.lidar_augment_workspace_bytes(2, 3, 15, 1000), L.lidar_augment_workspace_bytes(2, 3, 15, 100000)
    assert 0 < small < big and big >= 100000


def _call_args(B=2, C=4, M=8, n=10):
    pts = torch.zeros((n, C))
    offs = torch.tensor([0] + [n] * B, dtype=torch.int32)
    return pts, offs, torch.zeros((B, M, 8)), torch.zeros(B, dtype=torch.int32)


def test_wrapper_refusals():
    db = augment.GtDatabase(np.zeros((6, 4), np.float32), [0, 2, 6], np.ones((2, 7), np.float32), [1, 2], device="cpu")
    aug = augment.TrainAugmentor(db, 3, anp.KITTI_RANGE)
    pts, offs, gt, cnt = _call_args()
    cand = np.full((2, 3, 15), -1, np.int32)
    kw = dict(flip_x=np.zeros(2), flip_y=np.zeros(2), rot=np.zeros(2), scale=np.ones(2))
    bad = [
        ((pts.double(), offs, gt, cnt, cand), "float64 points"), ((pts[:, :3].contiguous(), offs, gt, cnt, cand), "C differs from the db"),
        ((pts, offs.long(), gt, cnt, cand), "int64 offsets"), ((pts, offs, gt[:, :, :7].contiguous(), cnt, cand), "7-column gt"),
        ((pts, offs, gt[:1], cnt, cand), "gt batch"), ((pts, offs, gt, cnt.long(), cand), "int64 counts"),
        ((pts, offs, gt, cnt[:1], cand), "counts shape"), ((pts, offs, gt, cnt, cand[:, :2]), "G differs"),
        ((pts, offs, gt, cnt, cand.astype(np.float32)), "float cand"), ((pts, offs, gt, cnt, np.full((2, 3, 65), -1, np.int32)), "S = 65"),
        ((pts, offs, torch.zeros((2, 468, 8)), cnt, cand), "M + G S = 513"),
    ]
    for args, what in bad:
        with pytest.raises(_lib.LidarHipError):
            aug(*args, **kw)
            pytest.fail(what)
    c2 = cand.copy()
    c2[0, 0, 0] = 2                                       # index >= n_obj
    with pytest.raises(_lib.LidarHipError, match="outside"):
        aug(pts, offs, gt, cnt, c2, **kw)
    c2[0, 0, 0] = 1                                       # object 1 has 4 points: the bound is 10 + 4
    with pytest.raises(_lib.LidarHipError, match="cap"):
        aug(pts, offs, gt, cnt, c2, cap=13, **kw)
    with pytest.raises(_lib.LidarHipError, match="CUDA"):            # at the limits and with cap == bound only the device is missing
        aug(pts, offs, torch.zeros((2, 467, 8)), cnt, c2, cap=14, **kw)
    with pytest.raises(_lib.LidarHipError, match="CUDA"):
        aug(pts, offs, torch.zeros((2, 512 - 3 * 64, 8)), cnt, np.full((2, 3, 64), -1, np.int32), **kw)
    with pytest.raises(_lib.LidarHipError):
        augment.TrainAugmentor(db, 3, anp.KITTI_RANGE, flip_axes="xz")
    with pytest.raises(_lib.LidarHipError):
        augment.DbSampler(db, [(1, 65)])
    with pytest.raises(_lib.LidarHipError):
        augment.DbSampler(db, [(1, 1)] * 9)


def test_draws_follow_the_reference_distributions():
    db = augment.GtDatabase(np.zeros((6, 4), np.float32), [0, 2, 6], np.ones((2, 7), np.float32), [1, 2], device="cpu")
    aug = augment.TrainAugmentor(db, 3, anp.KITTI_RANGE, world_rot_range=0.5, world_scale_range=(0.9, 1.1), flip_axes="x",
                                 sample_rot_range=(-0.2, 0.2))
    d = aug.draw(4000, 2, np.random.default_rng(0))
    assert set(np.unique(d["flip_x"])) == {0, 1} and not d["flip_y"].any() and abs(d["flip_x"].mean() - 0.5) < 0.05
    assert -0.5 <= d["rot"].min() < -0.45 and 0.45 < d["rot"].max() <= 0.5
    assert 0.9 <= d["scale"].min() < 0.91 and 1.09 < d["scale"].max() <= 1.1
    assert d["sample_rot"].shape == (4000, 3, 2) and np.abs(d["sample_rot"]).max() <= 0.2
    fixed = augment.TrainAugmentor(db, 3, anp.KITTI_RANGE, world_scale_range=(1.0, 1.0005))
    assert fixed.draw(3, 2, np.random.RandomState(0))["scale"] is None      # global_scaling returns early below 1e-3
