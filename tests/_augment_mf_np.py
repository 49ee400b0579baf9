"""Plain-numpy restatement of the pose path of lidar_augment_mf (include/lidar_hip.h): every gt's `locations` (S, 3) and `rotations_y`
(S) follow its box through GT sampling (road plane, sample rotation), the world flips, rotation and scaling, the range mask and the
compaction.  Shared by tests/test_augment_mf_host.py, tests/test_gpu_augment_mf.py and tools/augment_mf_bench.py.

Everything that decides something (collision test, carving, range mask, row order) is tests/_augment_np.py's, run unchanged; the
poses take no decision of their own, they are moved by the numbers that moved their box and kept where their box is kept.  The host
test pins this file to tests/golden/augment_mf_ref.npz, written by the reference itself: row counts and order exactly, floats to 1e-4.

Float32 arithmetic in the reference's op order (database_sampler.py:165-177, augmentor_utils.py:24-28, 51-55, 80-84, 105-107);
cos / sin as _augment_np takes them (in double, rounded once).  One declared divergence: a row with class id 0 leaves the poses as it
leaves the boxes, where the reference keeps its pose row and so loses the alignment of the two."""
import json
import os

import numpy as np

import _augment_np as anp

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_mf_ref.npz")
CASES = ["yaml3", "plane3", "single", "stack8"]
POSE_KEYS = ("locations", "rotations_y", "db_locations", "db_rotations_y")


def load_contract(name):
    """-> (cfg, inputs, expected, the whole file) of a case of augment_mf_ref.npz, with the road-plane 4-vectors of the contract added"""
    from lidardetection_amd.augment import road_plane_lidar
    z = np.load(GOLDEN)
    cfg = json.loads(str(z[f"{name}_cfg"]))
    inp = {k[len(name) + 4:]: z[k] for k in z.files if k.startswith(f"{name}_in_")}
    exp = {k[len(name) + 5:]: z[k] for k in z.files if k.startswith(f"{name}_out_")}
    if cfg["plane"]:
        inp["plane"] = np.stack([road_plane_lidar(z[f"{name}_rec_plane_abcd"][b], z[f"{name}_rec_V2C"][b], z[f"{name}_rec_R0"][b])
                                 for b in range(len(inp["rot"]))]).astype(F)
    return cfg, inp, exp, z


def without_poses(inp):
    return {k: v for k, v in inp.items() if k not in POSE_KEYS}


def sample_poses(loc, ry, box, plane, angle):
    """poses (S, 3), (S) of a database object as it joins the scene (database_sampler.py:165-177): box (7) its database box,
    plane (4,) or None, angle: its sample rotation or None"""
    loc, ry, b = loc.astype(F).copy(), ry.astype(F).copy(), box.astype(F).copy()
    if plane is not None:
        q = np.asarray(plane, F)
        mv = b[2] - b[5] / F(2) - (q[0] * b[0] + q[1] * b[1] + q[2] * b[2] + q[3])
        b[2] = b[2] - mv
        loc[:, 2] = loc[:, 2] - mv
    if angle is not None:
        ry = ry + F(angle)
        rc, rs = anp.cs_f32(angle)
        loc = loc - b[None, 0:3]
        loc = anp.rotate_z(loc, rc, rs)
        loc = loc + b[None, 0:3]
    return loc, ry


def world_poses(loc, ry, flip_x, flip_y, rot, scale):
    """world flip x, flip y, rotation and scaling of (n, S, 3) / (n, S) poses; rotations_y is not folded"""
    loc, ry = loc.astype(F).copy(), ry.astype(F).copy()
    if flip_x:
        loc[..., 1] = -loc[..., 1]
        ry = -ry
    if flip_y:
        loc[..., 0] = -loc[..., 0]
        ry = -(ry + anp.PI_F)
    c, s = anp.cs_f32(rot)
    loc = anp.rotate_z(loc.reshape(-1, 3), c, s).reshape(loc.shape)
    ry = ry + F(rot)
    if scale is not None:
        loc = loc * F(scale)
    return loc, ry


def augment(inp, cfg, iou_fn=None):
    """_augment_np.augment's inputs plus locations (B, M, S, 3), rotations_y (B, M, S), db_locations (n_obj, S, 3), db_rotations_y
    (n_obj, S) -> its outputs plus locations (B, M + G * per_group, S, 3) and rotations_y (B, M + G * per_group, S), zero-padded"""
    trace = []
    out = anp.augment(without_poses(inp), cfg, iou_fn, trace)
    B, G, P = inp["cand"].shape
    M, S = inp["gt_boxes"].shape[1], inp["locations"].shape[2]
    out_loc, out_ry = np.zeros((B, M + G * P, S, 3), F), np.zeros((B, M + G * P, S), F)
    for b in range(B):
        n = int(inp["gt_counts"][b])
        trained = np.nonzero(inp["gt_boxes"][b, :n, 7].astype(np.int32) > 0)[0]
        loc, ry = [inp["locations"][b, trained].astype(F)], [inp["rotations_y"][b, trained].astype(F)]
        for g in range(G):
            for k in range(P):
                if out["sample_valid"][b, g, k]:
                    c = int(inp["cand"][b, g, k])
                    l, r = sample_poses(inp["db_locations"][c], inp["db_rotations_y"][c], inp["db_boxes"][c],
                                        inp["plane"][b] if inp.get("plane") is not None else None,
                                        inp["sample_rot"][b, g, k] if inp.get("sample_rot") is not None else None)
                    loc.append(l[None])
                    ry.append(r[None])
        loc, ry = world_poses(np.concatenate(loc, 0), np.concatenate(ry, 0), int(inp["flip_x"][b]), int(inp["flip_y"][b]), inp["rot"][b],
                              inp["scale"][b] if cfg.get("apply_scale", True) else None)
        boxes = trace[b]["boxes"]                      # every row before the range mask: the poses stay where their box stays
        assert len(boxes) == len(loc)
        if cfg.get("remove_outside_boxes", True):
            keep = anp.box_corners_inside(boxes, np.asarray(cfg["pc_range"], F)) >= cfg.get("min_num_corners", 1)
            loc, ry = loc[keep], ry[keep]
        assert len(loc) == out["gt_counts"][b]
        out_loc[b, :len(loc)], out_ry[b, :len(ry)] = loc, ry
    out.update(locations=out_loc, rotations_y=out_ry)
    return out


def borderline_clear(inp, cfg, iou_fn=None):
    """the golden file's borderline condition: _augment_np's, nothing added — the poses take no decision"""
    return anp.borderline_clear(without_poses(inp), cfg, iou_fn)


def moved_poses(r, boxes, frames, shift=0.8, turn=0.3):
    """poses for `frames` stacked sweeps of (..., 7+) boxes: sweep 0 is the box's own pose, later sweeps drift and turn"""
    b = np.asarray(boxes, F)
    lead = b.shape[:-1]
    step = np.cumsum(r.normal(0, 1, (*lead, frames, 3)) * np.asarray([shift, shift, 0.05]), axis=-2)
    dturn = np.cumsum(r.normal(0, turn, (*lead, frames)), axis=-1)
    step[..., 0, :], dturn[..., 0] = 0, 0
    return (b[..., None, 0:3] + step).astype(F), (b[..., None, 6] + dturn).astype(F)


def add_poses(inp, frames, seed=0):
    """a copy of _augment_np.synth_inputs' inputs with poses for `frames` sweeps; rows past gt_counts get finite junk, which a call
    must ignore"""
    r = np.random.default_rng(seed)
    out = dict(inp)
    out["locations"], out["rotations_y"] = moved_poses(r, inp["gt_boxes"], frames)
    out["db_locations"], out["db_rotations_y"] = moved_poses(r, inp["db_boxes"], frames)
    for b, n in enumerate(inp["gt_counts"]):
        out["locations"][b, n:], out["rotations_y"][b, n:] = 77.0, -5.0
    return out


def pose_close(got, exp):
    return anp.close(got["locations"], exp["locations"]) and anp.close(got["rotations_y"], exp["rotations_y"])
