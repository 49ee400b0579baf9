"""Generates tests/golden/augment_mf_ref.npz from the REFERENCE ITSELF, by the method of make_augment_golden.py (whose loader, stubs,
recorder and float64 borderline checks are imported, not copied): the reference's own DataBaseSampler, augmentor_utils,
DataAugmentor.forward, DataProcessor.mask_points_and_boxes_outside_range and the `selected` step of DatasetTemplate.prepare_data
(pcdet/datasets/dataset.py:132-142) run on the CPU on synthetic frames whose data dicts and database infos carry the multi-frame extras
`locations` (n, S, 3) and `rotations_y` (n, S), cast to float32 before the reference sees them.  Runs only where the reference checkout
is (default /root/reference, or $LIDAR_REFERENCE); the .npz holds inputs, recorded draws and outputs.

What is NOT the reference: the same two compiled calls are stubs (see make_augment_golden.py), and the class-id column is added as
prepare_data adds it.  The same borderline condition applies; a seed that misses it, or in which not every situation occurs, is skipped.

The frames hold trained classes only.  With an untrained annotation the reference's pose rows stop lining up with its box rows
(add_sampled_boxes_to_scene masks gt_boxes but concatenates onto the unmasked locations; DataAugmentor.forward masks boxes and names
only), so there is nothing well defined to record; the generator asserts that every frame's output pose rows equal its box count.

Cases (B <= 4, frames <= 700 points, objects <= 48 points, M = 8, groups * per_group = 2 * 12: Car:12, Truck:8)
  yaml3   S = 3, pv_rcnn_multiframe.yaml-like: Car / Truck, C = 5, flip x, rotation, scaling
  plane3  S = 3, USE_ROAD_PLANE, SAMPLE_ROT_ANGLE, flips on both axes
  single  S = 1
  stack8  S = 8
Every case: a frame with no annotations, a frame where every candidate collides (eight strips of annotation cover the whole range), and
a frame where the range mask drops an input row and a pasted row (asserted on the reference's output).

Usage:  python tests/golden/make_augment_mf_golden.py
"""
import json
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_augment_golden as base  # noqa: E402
from _augment_mf_np import moved_poses  # noqa: E402
from oracle import c_oracle  # noqa: E402

Cfg, PC_RANGE = base.Cfg, base.PC_RANGE
CLASSES = ["Car", "Truck"]
SIZES = {"Car": [3.9, 1.6, 1.56], "Truck": [7.5, 2.4, 2.6]}
N_DB = {"Car": 16, "Truck": 12}
GROUPS = [("Car", 12), ("Truck", 8)]


def make_db(r, C, S):
    pts, offs, boxes, cls, names = [], [0], [], [], []
    for ci, name in enumerate(CLASSES):
        for j in range(N_DB[name]):
            size = np.array(SIZES[name]) * r.uniform(0.9, 1.1, 3)
            box = [r.uniform(6, 64), r.uniform(-36, 36), r.uniform(-1.2, -0.9), *size, r.uniform(-np.pi, np.pi)]
            if j in (1, 3):          # on top of the previous object: the two collide with each other wherever both are candidates
                box[0:2] = boxes[-1][0] + r.uniform(-0.3, 0.3), boxes[-1][1] + r.uniform(-0.3, 0.3)
            n = int(r.integers(0 if j == 5 else 4, 49))
            local = (r.uniform(-0.5, 0.5, (n, 3)) * size).astype(np.float32)
            pts.append(np.concatenate([local, r.uniform(0, 1, (n, C - 3)).astype(np.float32)], 1))
            offs.append(offs[-1] + n)
            boxes.append(np.array(box, np.float32))
            cls.append(ci + 1)
            names.append(name)
    boxes = np.stack(boxes)
    loc, ry = moved_poses(r, boxes, S)
    difficulty = np.array([int(i % 3) - (1 if i % 7 == 0 else 0) for i in range(len(boxes))], np.int32)
    return dict(points=np.concatenate(pts, 0), offsets=np.array(offs, np.int32), boxes=boxes, cls=np.array(cls, np.int32), names=names,
                difficulty=difficulty, locations=loc.astype(np.float32), rotations_y=ry.astype(np.float32))


def write_db(db, root):
    infos = {n: [] for n in CLASSES}
    for i, name in enumerate(db["names"]):
        path = f"gt_database/{i:04d}_{name}.bin"
        p = db["points"][db["offsets"][i]:db["offsets"][i + 1]]
        p.astype(np.float32).tofile(str(root / path))
        infos[name].append(dict(name=name, path=path, gt_idx=i, box3d_lidar=db["boxes"][i].copy(), num_points_in_gt=len(p),
                                difficulty=int(db["difficulty"][i]), gidx=i, locations=db["locations"][i].copy(),
                                rotations_y=db["rotations_y"][i].copy()))
    with open(root / "dbinfos.pkl", "wb") as f:
        pickle.dump(infos, f)


def make_frame(r, C, S, n_pts, kind, db):
    """-> (points (n, C), gt_boxes (k, 7), gt_names (k,), locations (k, S, 3), rotations_y (k, S)); trained classes only"""
    xyz = np.stack([r.uniform(-4, 74, n_pts), r.uniform(-44, 44, n_pts), r.uniform(-2.2, 0.4, n_pts)], 1)
    for i in r.choice(len(db["boxes"]), 20, replace=False):      # points inside database boxes: a pasted object has something to carve
        b = db["boxes"][i]
        xyz[int(r.integers(0, n_pts))] = [b[0] + r.uniform(-0.2, 0.2), b[1] + r.uniform(-0.2, 0.2), b[2] + r.uniform(-0.3, 0.3)]
    pts = np.concatenate([xyz, r.uniform(0, 1, (n_pts, C - 3))], 1).astype(np.float32)
    boxes, names = [], []
    if kind == "blocked":            # eight strips of annotation over the whole range: every database object touches one
        for j in range(8):
            boxes.append([34.5, -36.75 + 10.5 * j, -1.0, 68.0, 10.5, 1.6, r.uniform(-0.004, 0.004)])
            names.append(CLASSES[j % 2])
    elif kind == "mixed":
        for j in range(int(r.integers(3, 7))):
            name = CLASSES[int(r.integers(0, 2))]
            boxes.append([r.uniform(6, 60), r.uniform(-30, 30), r.uniform(-1.2, -0.9), *(np.array(SIZES[name]) * r.uniform(0.9, 1.1, 3)),
                          r.uniform(-np.pi, np.pi)])
            names.append(name)
        for sy in (1, -1):           # near the far corners of the range: the world rotation takes them out of it
            boxes.append([r.uniform(65, 67), sy * r.uniform(35, 37), -1.0, *SIZES["Car"], r.uniform(-np.pi, np.pi)])
            names.append("Car")
        order = r.permutation(len(boxes))
        boxes, names = [boxes[i] for i in order], [names[i] for i in order]
    boxes = np.array(boxes, np.float32).reshape(-1, 7)
    loc, ry = moved_poses(r, boxes, S)
    return pts, boxes, np.array(names, dtype="<U12"), loc.astype(np.float32), ry.astype(np.float32)


def run_case(m, spec, seed):
    """-> (cfg, arrays) for the file, or None when a decision is borderline or a situation is missing"""
    r = np.random.default_rng(seed)
    C, S, kinds = spec["C"], spec["S"], spec["frames"]
    B, G, P = len(kinds), len(GROUPS), max(n for _, n in GROUPS)
    db = make_db(r, C, S)
    frames = [make_frame(r, C, S, int(r.integers(500, 701)), kind, db) for kind in kinds]
    M = 8
    assert all(len(f[1]) <= M for f in frames)
    sampler_cfg = Cfg(NAME="gt_sampling", USE_ROAD_PLANE=spec.get("plane", False), DB_INFO_PATH=["dbinfos.pkl"],
                      PREPARE=Cfg(filter_by_min_points=["Car:1", "Truck:1"], filter_by_difficulty=[-1]),
                      SAMPLE_GROUPS=[f"{n}:{k}" for n, k in GROUPS], NUM_POINT_FEATURES=C, DATABASE_WITH_FAKELIDAR=False,
                      REMOVE_EXTRA_WIDTH=spec.get("remove_extra_width", [0.0, 0.0, 0.0]), LIMIT_WHOLE_SCENE=False)
    if "sample_rot" in spec:
        sampler_cfg["SAMPLE_ROT_ANGLE"] = spec["sample_rot"]
    aug_cfg = Cfg(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=[
        sampler_cfg, Cfg(NAME="random_world_flip", ALONG_AXIS_LIST=spec["flip"]),
        Cfg(NAME="random_world_rotation", WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
        Cfg(NAME="random_world_scaling", WORLD_SCALE_RANGE=[0.95, 1.05])])
    out = dict(cand=np.full((B, G, P), -1, np.int32), flip_x=np.zeros(B, np.int32), flip_y=np.zeros(B, np.int32), rot=np.zeros(B, np.float32),
               scale=np.zeros(B, np.float32), sample_rot=np.zeros((B, G, P), np.float32), sample_valid=np.zeros((B, G, P), np.int32),
               plane_abcd=np.zeros((B, 4), np.float64), V2C=np.zeros((B, 3, 4), np.float32), R0=np.zeros((B, 3, 3), np.float32))
    perms, clear = [], [True]
    res_pts, res_boxes, res_loc, res_ry = [], [], [], []
    stats = dict(accepted=0, rejected=0, carved=0, range_dropped_input=0, range_dropped_pasted=0, frames_dropping_both=0)
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        (root / "gt_database").mkdir()
        write_db(db, root)
        np.random.seed(seed)
        augmentor = m["augmentor"].DataAugmentor(root, aug_cfg, CLASSES)
        sampler = augmentor.data_augmentor_queue[0]
        processor = m["processor"].DataProcessor([], np.array(PC_RANGE, np.float32), training=True)
        state = {}
        inner_sample = sampler.sample_with_fixed_number

        def sample_with_fixed_number(class_name, sample_group):
            got = inner_sample(class_name, sample_group)
            g = [n for n, _ in GROUPS].index(class_name)
            out["cand"][state["b"], g, :len(got)] = [info["gidx"] for info in got]
            return got

        sampler.sample_with_fixed_number = sample_with_fixed_number
        inner_add = sampler.add_sampled_boxes_to_scene

        def add_sampled_boxes_to_scene(data_dict, sampled_gt_boxes, total_valid_sampled_dict):
            state["valid"] = [info["gidx"] for info in total_valid_sampled_dict]
            return inner_add(data_dict, sampled_gt_boxes, total_valid_sampled_dict)

        sampler.add_sampled_boxes_to_scene = add_sampled_boxes_to_scene
        inner_remove = m["box_utils"].remove_points_in_boxes3d

        def remove_points_in_boxes3d(points, boxes3d):
            clear[0] &= base.carve_clear(points[:, 0:3], boxes3d.numpy() if torch.is_tensor(boxes3d) else boxes3d)
            kept = inner_remove(points, boxes3d)
            stats["carved"] += len(points) - len(kept)
            return kept

        m["box_utils"].remove_points_in_boxes3d = remove_points_in_boxes3d
        try:
            for b, (pts, boxes, names, loc, ry) in enumerate(frames):
                state.update(b=b, valid=[])
                calib, V2C, R0 = base.make_calib(r, m)
                plane = np.array([r.normal(0, 0.01), -1.0, r.normal(0, 0.01), r.uniform(1.5, 1.8)])
                out["plane_abcd"][b], out["V2C"][b], out["R0"][b] = plane, V2C, R0
                data = dict(points=pts.copy(), gt_boxes=boxes.copy(), gt_names=names.copy(), locations=loc.astype(np.float32).copy(),
                            rotations_y=ry.astype(np.float32).copy(), gt_boxes_mask=np.array([n in CLASSES for n in names], dtype=np.bool_))
                assert data["gt_boxes_mask"].all()
                if spec.get("plane", False):
                    data.update(road_plane=plane, calib=calib)
                with base.Recorder() as rec:
                    data = augmentor.forward(data)
                events = list(rec.events)
                perms += [e[1] for e in events if e[0] == "perm"]
                events = [e for e in events if e[0] != "perm"]
                n_valid = len(state["valid"])
                if "sample_rot" in spec and n_valid:
                    kind, v = events.pop(0)
                    assert kind == "uniform" and v.shape == (n_valid,)
                    where = {int(g): k for k, g in enumerate(state["valid"])}
                    for g in range(G):
                        for s in range(P):
                            if out["cand"][b, g, s] >= 0 and int(out["cand"][b, g, s]) in where:
                                out["sample_rot"][b, g, s] = v[where[int(out["cand"][b, g, s])]]
                for axis in spec["flip"]:
                    kind, v = events.pop(0)
                    assert kind == "choice"
                    out["flip_" + axis][b] = v
                (k1, rot), (k2, scale) = events
                assert k1 == "uniform" and k2 == "uniform"
                out["rot"][b], out["scale"][b] = rot, scale
                for g in range(G):
                    for s in range(P):
                        out["sample_valid"][b, g, s] = int(out["cand"][b, g, s] >= 0 and int(out["cand"][b, g, s]) in state["valid"])
                # the collision tests' pairs, group by group, in float64
                existing = boxes.reshape(-1, 7)
                for g in range(G):
                    live = out["cand"][b, g][out["cand"][b, g] >= 0]
                    cb = db["boxes"][live]
                    clear[0] &= base.pairs_clear(cb, existing)
                    ok = out["sample_valid"][b, g][out["cand"][b, g] >= 0].astype(bool)
                    if len(live):
                        own = c_oracle.pairwise(cb, cb, 1)
                        np.fill_diagonal(own, 0)
                        hit_old = (c_oracle.pairwise(cb, existing, 1) > 0).any(axis=1) if len(existing) else np.zeros(len(live), bool)
                        assert np.array_equal(ok, ~((own.max(axis=1) > 0) | hit_old)), "the replayed collision test differs from the reference's"
                    existing = np.concatenate([existing, cb[ok]], 0)
                    stats["accepted"] += int(ok.sum())
                    stats["rejected"] += int((~ok).sum())
                # DatasetTemplate.prepare_data between the augmentor and the processor (dataset.py:132-142)
                selected = m["common_utils"].keep_arrays_by_name(data["gt_names"], CLASSES)
                data["gt_boxes"], data["gt_names"] = data["gt_boxes"][selected], data["gt_names"][selected]
                gt_classes = np.array([CLASSES.index(n) + 1 for n in data["gt_names"]], dtype=np.int32)
                data["gt_boxes"] = np.concatenate((data["gt_boxes"], gt_classes.reshape(-1, 1).astype(np.float32)), axis=1)
                data["locations"], data["rotations_y"] = data["locations"][selected], data["rotations_y"][selected]
                assert len(data["gt_boxes"]) == len(boxes) + n_valid == len(data["locations"]) == len(data["rotations_y"])
                assert data["locations"].dtype == np.float32 and data["rotations_y"].dtype == np.float32
                clear[0] &= base.range_clear(data["points"], data["gt_boxes"])
                inside = m["box_utils"].mask_boxes_outside_range_numpy(data["gt_boxes"], np.array(PC_RANGE, np.float32), min_num_corners=1)
                data = processor.mask_points_and_boxes_outside_range(data_dict=data, config=Cfg(REMOVE_OUTSIDE_BOXES=True, min_num_corners=1))
                # the reference's output pose rows equal its box count, and they are the rows the range mask kept
                assert len(data["gt_boxes"]) == len(data["locations"]) == len(data["rotations_y"]) == int(inside.sum())
                d_in, d_paste = int((~inside[:len(boxes)]).sum()), int((~inside[len(boxes):]).sum())
                stats["range_dropped_input"] += d_in
                stats["range_dropped_pasted"] += d_paste
                stats["frames_dropping_both"] += int(d_in > 0 and d_paste > 0)
                res_pts.append(np.asarray(data["points"], np.float32))
                res_boxes.append(np.asarray(data["gt_boxes"], np.float32).reshape(-1, 8))
                res_loc.append(np.asarray(data["locations"], np.float32).reshape(-1, S, 3))
                res_ry.append(np.asarray(data["rotations_y"], np.float32).reshape(-1, S))
                if not clear[0]:
                    return None
                if kinds[b] == "blocked" and (n_valid or not (out["cand"][b] >= 0).any()):
                    return None          # the strips must stop every candidate
        finally:
            m["box_utils"].remove_points_in_boxes3d = inner_remove
    if stats["accepted"] == 0 or stats["rejected"] == 0 or stats["carved"] == 0 or stats["frames_dropping_both"] == 0:
        print(f"   seed {seed}: not every situation occurs: {stats}")
        return None
    T = G * P
    gt_in, gt_out = np.zeros((B, M, 8), np.float32), np.zeros((B, M + T, 8), np.float32)
    loc_in, ry_in = np.zeros((B, M, S, 3), np.float32), np.zeros((B, M, S), np.float32)
    loc_out, ry_out = np.zeros((B, M + T, S, 3), np.float32), np.zeros((B, M + T, S), np.float32)
    for b, (pts, boxes, names, loc, ry) in enumerate(frames):
        k = len(boxes)
        gt_in[b, :k, :7], gt_in[b, :k, 7] = boxes, [CLASSES.index(n) + 1 for n in names]
        loc_in[b, :k], ry_in[b, :k] = loc, ry
        n = len(res_boxes[b])
        gt_out[b, :n], loc_out[b, :n], ry_out[b, :n] = res_boxes[b], res_loc[b], res_ry[b]
    res = dict(
        in_points=np.concatenate([f[0] for f in frames], 0), in_point_offsets=np.cumsum([0] + [len(f[0]) for f in frames]).astype(np.int32),
        in_gt_boxes=gt_in, in_gt_counts=np.array([len(f[1]) for f in frames], np.int32), in_locations=loc_in, in_rotations_y=ry_in,
        in_db_points=db["points"], in_db_offsets=db["offsets"], in_db_boxes=db["boxes"], in_db_cls=db["cls"],
        in_db_locations=db["locations"], in_db_rotations_y=db["rotations_y"], in_cand=out["cand"], in_flip_x=out["flip_x"],
        in_flip_y=out["flip_y"], in_rot=out["rot"], in_scale=out["scale"],
        out_points=np.concatenate(res_pts, 0), out_point_offsets=np.cumsum([0] + [len(p) for p in res_pts]).astype(np.int32),
        out_gt_boxes=gt_out, out_gt_counts=np.array([len(x) for x in res_boxes], np.int32), out_sample_valid=out["sample_valid"],
        out_locations=loc_out, out_rotations_y=ry_out,
        rec_perms=np.concatenate(perms).astype(np.int32) if perms else np.zeros(0, np.int32),
        rec_perm_len=np.array([len(p) for p in perms], np.int32), rec_db_difficulty=db["difficulty"])
    if "sample_rot" in spec:
        res["in_sample_rot"] = out["sample_rot"]
    if spec.get("plane", False):
        res.update(rec_plane_abcd=out["plane_abcd"], rec_V2C=out["V2C"], rec_R0=out["R0"])
    cfg = dict(remove_extra_width=spec.get("remove_extra_width", [0.0, 0.0, 0.0]), collide_extra_width=None, pc_range=PC_RANGE,
               remove_outside_boxes=True, min_num_corners=1, apply_scale=True, groups=[[CLASSES.index(n) + 1, k] for n, k in GROUPS],
               removed_difficulty=[-1], min_points={"1": 1, "2": 1}, flip=spec["flip"], plane=spec.get("plane", False),
               stack_frames=S, frames=kinds, stats=stats)
    return cfg, res



CASES = {
    "yaml3": dict(C=5, S=3, frames=["mixed", "empty", "blocked", "mixed"], flip=["x"]),
    "plane3": dict(C=4, S=3, frames=["mixed", "empty", "blocked", "mixed"], flip=["x", "y"], plane=True, sample_rot=[-0.3, 0.3],
                   remove_extra_width=[0.2, 0.2, 0.1]),
    "single": dict(C=4, S=1, frames=["mixed", "empty", "blocked"], flip=["x"]),
    "stack8": dict(C=4, S=8, frames=["mixed", "empty", "blocked"], flip=["x"]),
}


def main():
    m = base.load_reference()
    out = {}
    for name, spec in CASES.items():
        for seed in range(900, 1400):
            got = run_case(m, spec, seed)
            if got is not None:
                break
        else:
            raise RuntimeError(f"{name}: no seed keeps every decision clear of its threshold")
        cfg, res = got
        print(f"{name}: seed {seed}, {cfg['stats']}, points {res['in_point_offsets'][-1]} -> {res['out_point_offsets'][-1]}, "
              f"boxes {res['in_gt_counts'].tolist()} -> {res['out_gt_counts'].tolist()}")
        out[f"{name}_cfg"] = np.array(json.dumps(cfg))
        for k, v in res.items():
            out[f"{name}_{k}"] = v
    path = os.path.join(HERE, "augment_mf_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
