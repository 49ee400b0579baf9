"""Generates tests/golden/augment_ref.npz from the REFERENCE ITSELF: its own DataBaseSampler (__call__ / add_sampled_boxes_to_scene),
augmentor_utils, DataAugmentor.forward, DataProcessor.mask_points_and_boxes_outside_range and calibration_kitti, loaded standalone
from their files and run on synthetic frames on the CPU.  Runs only where the reference checkout is (default /root/reference, or
$LIDAR_REFERENCE); the .npz (inputs, recorded random numbers, outputs) is what the tests read.

What is NOT the reference:
  * its two compiled CPU calls are stubs: iou3d_nms_utils.boxes_bev_iou_cpu is oracle.c_oracle.pairwise(a, b, 1), the mode
    tests/test_oracle_pins.py pins to the reference-compiled code, and roiaware_pool3d_utils.points_in_boxes_cpu is
    oracle.c_oracle.points_in_boxes_cpu;
  * between DataAugmentor.forward and the DataProcessor the generator does what DatasetTemplate.prepare_data does there
    (pcdet/datasets/dataset.py:132-138): common_utils.keep_arrays_by_name (the reference's) and the class-id column.

The generator writes a synthetic database (pickle + .bin files) into a temporary directory.  np.random.permutation, uniform and choice
are wrapped while the reference runs; the wrappers pass the arguments through, return the real draws and record them; the file stores
them as the contract's inputs (cand, flip_x, flip_y, rot, scale, sample_rot) plus the permutations themselves (for DbSampler) and the
heights put_boxes_on_road_planes returned (for road_plane_lidar).

Borderline condition, so that index results compare exactly with nothing left out.  The decisions are evaluated in float64 and the
generator moves to the next seed unless: every box pair of a collision test has reference IoU >= 1e-3 or a separating-axis gap
>= 3e-2 (the issue asks 1e-2; the clipper's own corner margin is 1e-2, so the generator keeps clear of it too); no scene point lies
within 1e-3 of a face of a carving box (margin included) and no point within 1e-3 of an x / y range limit; no box corner lies within
1e-3 of a range limit; no heading lies within 1e-3 of the +-pi fold of limit_period.

Cases (frames <= 1200 points, objects <= 48 points, B <= 4)
  kitti     pointpillar.yaml: USE_ROAD_PLANE, Car:15 Pedestrian:10 Cyclist:10, REMOVE_EXTRA_WIDTH 0, flip x.  frame 0: trained and
            untrained ("Van") annotations, the Vans on top of database objects; frame 1: no annotations; frame 2: an annotation on top of
            every database object, so every candidate collides; frame 3: annotations again.  The 20 database cars make the pointer wrap.
  wide      REMOVE_SAMPLE_BOXES_EXTRA_WIDTH, REMOVE_EXTRA_WIDTH, SAMPLE_ROT_ANGLE, flips on both axes
  limit     LIMIT_WHOLE_SCENE
  feat5     C = 5
  corners8  min_num_corners 8
Every database has pairs of objects on top of each other (two candidates that collide only with each other are both dropped).

Usage:  python tests/golden/make_augment_golden.py
"""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refpcdet_aug"

from oracle import c_oracle  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
SIZES = {"Car": [3.9, 1.6, 1.56], "Pedestrian": [0.8, 0.6, 1.73], "Cyclist": [1.76, 0.6, 1.73], "Van": [5.0, 1.9, 2.2]}
PC_RANGE = [0.0, -39.68, -3.0, 69.12, 39.68, 1.0]
N_DB = {"Car": 20, "Pedestrian": 14, "Cyclist": 14}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def load_reference():
    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    root = os.path.join(REF, "pcdet")
    for sub in ["", ".utils", ".ops", ".ops.iou3d_nms", ".ops.roiaware_pool3d", ".datasets", ".datasets.augmentor", ".datasets.processor"]:
        pkg(PKG + sub, os.path.join(root, *sub.split(".")[1:]))
    sys.modules.setdefault("quaternion", types.ModuleType("quaternion"))
    iou = types.ModuleType(PKG + ".ops.iou3d_nms.iou3d_nms_utils")
    iou.boxes_bev_iou_cpu = lambda a, b: c_oracle.pairwise(np.asarray(a, np.float32).reshape(-1, 7), np.asarray(b, np.float32).reshape(-1, 7), 1)
    pib = types.ModuleType(PKG + ".ops.roiaware_pool3d.roiaware_pool3d_utils")
    pib.points_in_boxes_cpu = lambda points, boxes: torch.from_numpy(
        c_oracle.points_in_boxes_cpu(boxes.float().numpy(), points.float().numpy()))
    sys.modules[iou.__name__], sys.modules[pib.__name__] = iou, pib
    sys.modules[PKG + ".ops.iou3d_nms"].iou3d_nms_utils = iou
    sys.modules[PKG + ".ops.roiaware_pool3d"].roiaware_pool3d_utils = pib
    m = {}
    m["common_utils"] = load(PKG + ".utils.common_utils", os.path.join(root, "utils", "common_utils.py"))
    sys.modules[PKG + ".utils"].common_utils = m["common_utils"]
    m["box_utils"] = load(PKG + ".utils.box_utils", os.path.join(root, "utils", "box_utils.py"))
    sys.modules[PKG + ".utils"].box_utils = m["box_utils"]
    m["calib"] = load(PKG + ".utils.calibration_kitti", os.path.join(root, "utils", "calibration_kitti.py"))
    aug = os.path.join(root, "datasets", "augmentor")
    m["augmentor_utils"] = load(PKG + ".datasets.augmentor.augmentor_utils", os.path.join(aug, "augmentor_utils.py"))
    sys.modules[PKG + ".datasets.augmentor"].augmentor_utils = m["augmentor_utils"]
    m["sampler"] = load(PKG + ".datasets.augmentor.database_sampler", os.path.join(aug, "database_sampler.py"))
    sys.modules[PKG + ".datasets.augmentor"].database_sampler = m["sampler"]
    m["augmentor"] = load(PKG + ".datasets.augmentor.data_augmentor", os.path.join(aug, "data_augmentor.py"))
    m["processor"] = load(PKG + ".datasets.processor.data_processor", os.path.join(root, "datasets", "processor", "data_processor.py"))
    return m


# ---------------------------------------------------------------- synthetic data
def make_db(r, C):
    """-> dict(points, offsets, boxes, cls, names): objects scattered over the range, each class with two pairs on top of each other"""
    pts, offs, boxes, cls, names = [], [0], [], [], []
    for ci, name in enumerate(CLASSES):
        first = len(boxes)
        for j in range(N_DB[name]):
            size = np.array(SIZES[name]) * r.uniform(0.9, 1.1, 3)
            box = [r.uniform(4, 68), r.uniform(-38, 38), r.uniform(-1.2, -0.6), *size, r.uniform(-np.pi, np.pi)]
            if j in (1, 3):          # on top of the previous object: the two collide with each other wherever both are candidates
                box[0:2] = boxes[-1][0] + r.uniform(-0.3, 0.3), boxes[-1][1] + r.uniform(-0.3, 0.3)
            n = int(r.integers(0 if j == 5 else 4, 49))
            local = (r.uniform(-0.5, 0.5, (n, 3)) * size).astype(np.float32)
            pts.append(np.concatenate([local, r.uniform(0, 1, (n, C - 3)).astype(np.float32)], 1))
            offs.append(offs[-1] + n)
            boxes.append(np.array(box, np.float32))
            cls.append(ci + 1)
            names.append(name)
        assert len(boxes) - first == N_DB[name]
    difficulty = np.array([int(i % 3) - (1 if i % 7 == 0 else 0) for i in range(len(boxes))], np.int32)      # -1: objects 0, 21, 42
    return dict(points=np.concatenate(pts, 0), offsets=np.array(offs, np.int32), boxes=np.stack(boxes), cls=np.array(cls, np.int32),
                names=names, difficulty=difficulty)


def write_db(db, C, root):
    infos = {n: [] for n in CLASSES}
    for i, name in enumerate(db["names"]):
        path = f"gt_database/{i:04d}_{name}.bin"
        p = db["points"][db["offsets"][i]:db["offsets"][i + 1]]
        p.astype(np.float32).tofile(str(root / path))
        infos[name].append(dict(name=name, path=path, gt_idx=i, box3d_lidar=db["boxes"][i].copy(), num_points_in_gt=len(p),
                                difficulty=int(db["difficulty"][i]), gidx=i))
    with open(root / "dbinfos.pkl", "wb") as f:
        pickle.dump(infos, f)


def make_frame(r, C, n_pts, kind, db):
    """-> (points (n, C), gt_boxes (k, 7), gt_names (k,))"""
    xyz = np.stack([r.uniform(-4, 74, n_pts), r.uniform(-44, 44, n_pts), r.uniform(-2.2, 0.4, n_pts)], 1)
    # a few points inside database boxes, so that a pasted object always has something to carve
    for i in r.choice(len(db["boxes"]), 30, replace=False):
        b = db["boxes"][i]
        xyz[int(r.integers(0, n_pts))] = [b[0] + r.uniform(-0.2, 0.2), b[1] + r.uniform(-0.2, 0.2), b[2] + r.uniform(-0.3, 0.3)]
    pts = np.concatenate([xyz, r.uniform(0, 1, (n_pts, C - 3))], 1).astype(np.float32)
    boxes, names = [], []
    if kind == "empty":
        pass
    elif kind == "blocked":          # a trained annotation on top of every database object
        for i, b in enumerate(db["boxes"]):
            boxes.append([b[0] + r.uniform(-0.1, 0.1), b[1] + r.uniform(-0.1, 0.1), *b[2:7]])
            names.append(db["names"][i])
    else:
        for j in range(int(r.integers(4, 9))):
            name = CLASSES[int(r.integers(0, 3))] if kind != "cars" else "Car"
            boxes.append([r.uniform(4, 68), r.uniform(-38, 38), r.uniform(-1.2, -0.6), *(np.array(SIZES[name]) * r.uniform(0.9, 1.1, 3)),
                          r.uniform(-np.pi, np.pi)])
            names.append(name)
        for i in r.choice(N_DB["Car"], 4, replace=False):      # untrained annotations on top of database cars
            b = db["boxes"][i]
            boxes.append([b[0] + r.uniform(-0.5, 0.5), b[1] + r.uniform(-0.5, 0.5), -0.9, *SIZES["Van"], r.uniform(-np.pi, np.pi)])
            names.append("Van")
        order = r.permutation(len(boxes))
        boxes, names = [boxes[i] for i in order], [names[i] for i in order]
    return pts, np.array(boxes, np.float32).reshape(-1, 7), np.array(names, dtype="<U12")


def make_calib(r, m):
    rz = r.normal(0, 0.01, 3)
    V2C = np.array([[rz[0], -1.0, rz[1], 0.004], [rz[2], 0.01, -1.0, -0.076], [1.0, rz[0], 0.012, -0.272]], np.float32)
    R0 = (np.eye(3) + r.normal(0, 0.005, (3, 3))).astype(np.float32)
    P2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003]], np.float32)
    return m["calib"].Calibration(dict(P2=P2, R0=R0, Tr_velo2cam=V2C)), V2C, R0


# ---------------------------------------------------------------- float64 borderline checks
def corners2d(b):
    c, s = np.cos(b[6]), np.sin(b[6])
    local = np.array([[1, 1], [1, -1], [-1, -1], [-1, 1]], np.float64) * np.array([b[3], b[4]], np.float64) / 2
    return local @ np.array([[c, s], [-s, c]]) + np.array([b[0], b[1]], np.float64)


def sat_gap(a, b):
    """largest separation of the two rectangles along an axis of either (negative: they overlap)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    best = -np.inf
    for p, q in ((a, b), (b, a)):
        c, s = np.cos(p[6]), np.sin(p[6])
        rel = corners2d(q) - p[0:2]
        u, v = rel @ np.array([c, s]), rel @ np.array([-s, c])
        best = max(best, u.min() - p[3] / 2, -u.max() - p[3] / 2, v.min() - p[4] / 2, -v.max() - p[4] / 2)
    return best


def pairs_clear(cands, existing):
    """every pair a collision test can evaluate: candidates x (existing + candidates)"""
    if not len(cands):
        return True
    both = np.concatenate([existing, cands], 0)
    iou = c_oracle.pairwise(cands, both, 1)
    for i in range(len(cands)):
        for j in range(len(both)):
            if j == len(existing) + i:
                continue
            if not (iou[i, j] >= 1e-3 or (iou[i, j] == 0 and sat_gap(cands[i], both[j]) >= 3e-2)):
                return False
    return True


def carve_clear(points, boxes):
    p = np.asarray(points, np.float64)
    for b in np.asarray(boxes, np.float64):
        c, s = np.cos(-b[6]), np.sin(-b[6])
        sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
        lx, ly = sx * c - sy * s, sx * s + sy * c
        d = np.minimum(np.minimum(np.abs(np.abs(lx) - (b[3] / 2 + 1e-2)), np.abs(np.abs(ly) - (b[4] / 2 + 1e-2))),
                       np.abs(np.abs(p[:, 2] - b[2]) - b[5] / 2))
        near = (np.abs(lx) < b[3] / 2 + 0.02) & (np.abs(ly) < b[4] / 2 + 0.02) & (np.abs(p[:, 2] - b[2]) < b[5] / 2 + 0.01)
        if np.any(near & (d < 1e-3)):
            return False
    return True


def range_clear(points, boxes):
    p = np.asarray(points, np.float64)
    r = np.asarray(PC_RANGE, np.float64)
    for col, lo, hi in ((0, r[0], r[3]), (1, r[1], r[4])):
        if np.any(np.minimum(np.abs(p[:, col] - lo), np.abs(p[:, col] - hi)) < 1e-3):
            return False
    for b in np.asarray(boxes, np.float64):
        xy = corners2d(b)
        z = np.array([b[2] - b[5] / 2, b[2] + b[5] / 2])
        for vals, lo, hi in ((xy[:, 0], r[0], r[3]), (xy[:, 1], r[1], r[4]), (z, r[2], r[5])):
            if np.any(np.minimum(np.abs(vals - lo), np.abs(vals - hi)) < 1e-3):
                return False
        if np.pi - abs(b[6]) < 1e-3:
            return False
    return True


# ---------------------------------------------------------------- one case
class Recorder:
    def __init__(self):
        self.events = []

    def __enter__(self):
        self.saved = (np.random.permutation, np.random.uniform, np.random.choice)
        perm, uni, cho = self.saved

        def permutation(*a, **k):
            out = perm(*a, **k)
            self.events.append(("perm", np.array(out)))
            return out

        def uniform(*a, **k):
            out = uni(*a, **k)
            self.events.append(("uniform", np.array(out, np.float64)))
            return out

        def choice(*a, **k):
            out = cho(*a, **k)
            self.events.append(("choice", int(out)))
            return out

        np.random.permutation, np.random.uniform, np.random.choice = permutation, uniform, choice
        return self

    def __exit__(self, *exc):
        np.random.permutation, np.random.uniform, np.random.choice = self.saved


def run_case(m, spec, seed):
    """-> dict of arrays for the file, or None when a decision is borderline"""
    r = np.random.default_rng(seed)
    C, kinds, groups = spec["C"], spec["frames"], spec["groups"]
    B, G, S = len(kinds), len(groups), max(n for _, n in groups)
    db = make_db(r, C)
    frames = [make_frame(r, C, int(r.integers(900, 1201)), kind, db) for kind in kinds]
    M = max(8, max(len(f[1]) for f in frames))
    sampler_cfg = Cfg(NAME="gt_sampling", USE_ROAD_PLANE=spec.get("plane", False), DB_INFO_PATH=["dbinfos.pkl"],
                      PREPARE=Cfg(filter_by_min_points=["Car:5", "Pedestrian:0", "Cyclist:0"], filter_by_difficulty=[-1]),
                      SAMPLE_GROUPS=[f"{n}:{k}" for n, k in groups], NUM_POINT_FEATURES=C, DATABASE_WITH_FAKELIDAR=False,
                      REMOVE_EXTRA_WIDTH=spec.get("remove_extra_width", [0.0, 0.0, 0.0]), LIMIT_WHOLE_SCENE=spec.get("limit", False))
    if "collide_extra_width" in spec:
        sampler_cfg["REMOVE_SAMPLE_BOXES_EXTRA_WIDTH"] = spec["collide_extra_width"]
    if "sample_rot" in spec:
        sampler_cfg["SAMPLE_ROT_ANGLE"] = spec["sample_rot"]
    aug_cfg = Cfg(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=[
        sampler_cfg, Cfg(NAME="random_world_flip", ALONG_AXIS_LIST=spec["flip"]),
        Cfg(NAME="random_world_rotation", WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
        Cfg(NAME="random_world_scaling", WORLD_SCALE_RANGE=[0.95, 1.05])])
    out = dict(cand=np.full((B, G, S), -1, np.int32), flip_x=np.zeros(B, np.int32), flip_y=np.zeros(B, np.int32), rot=np.zeros(B, np.float32),
               scale=np.zeros(B, np.float32), sample_rot=np.zeros((B, G, S), np.float32), sample_valid=np.zeros((B, G, S), np.int32),
               plane_abcd=np.zeros((B, 4), np.float64), V2C=np.zeros((B, 3, 4), np.float32), R0=np.zeros((B, 3, 3), np.float32))
    perms, heights, clear = [], [], [True]
    res_pts, res_boxes, stats = [], [], dict(accepted=0, rejected=0, carved=0, only_untrained=0, only_each_other=0)
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        (root / "gt_database").mkdir()
        write_db(db, C, root)
        np.random.seed(seed)
        augmentor = m["augmentor"].DataAugmentor(root, aug_cfg, CLASSES)
        sampler = augmentor.data_augmentor_queue[0]
        processor = m["processor"].DataProcessor([], np.array(PC_RANGE, np.float32), training=True)
        state = {}
        inner_sample = sampler.sample_with_fixed_number

        def sample_with_fixed_number(class_name, sample_group):
            got = inner_sample(class_name, sample_group)
            g = [n for n, _ in groups].index(class_name)
            out["cand"][state["b"], g, :len(got)] = [info["gidx"] for info in got]
            return got

        sampler.sample_with_fixed_number = sample_with_fixed_number
        inner_add = sampler.add_sampled_boxes_to_scene

        def add_sampled_boxes_to_scene(data_dict, sampled_gt_boxes, total_valid_sampled_dict):
            state["valid"] = [info["gidx"] for info in total_valid_sampled_dict]
            return inner_add(data_dict, sampled_gt_boxes, total_valid_sampled_dict)

        sampler.add_sampled_boxes_to_scene = add_sampled_boxes_to_scene
        cls_sampler = m["sampler"].DataBaseSampler
        inner_plane = cls_sampler.put_boxes_on_road_planes

        def put_boxes_on_road_planes(gt_boxes, road_planes, calib):
            before = gt_boxes.copy()
            boxes, mv = inner_plane(gt_boxes, road_planes, calib)
            heights.append(np.concatenate([np.full((len(mv), 1), state["b"]), before[:, [0, 1, 2, 5]], np.asarray(mv).reshape(-1, 1)], 1))
            return boxes, mv

        cls_sampler.put_boxes_on_road_planes = staticmethod(put_boxes_on_road_planes)
        inner_remove = m["box_utils"].remove_points_in_boxes3d

        def remove_points_in_boxes3d(points, boxes3d):
            clear[0] &= carve_clear(points[:, 0:3], boxes3d.numpy() if torch.is_tensor(boxes3d) else boxes3d)
            kept = inner_remove(points, boxes3d)
            stats["carved"] += len(points) - len(kept)
            return kept

        m["box_utils"].remove_points_in_boxes3d = remove_points_in_boxes3d
        try:
            for b, (pts, boxes, names) in enumerate(frames):
                state.update(b=b, valid=[])
                calib, V2C, R0 = make_calib(r, m)
                plane = np.array([r.normal(0, 0.01), -1.0, r.normal(0, 0.01), r.uniform(1.5, 1.8)])
                out["plane_abcd"][b], out["V2C"][b], out["R0"][b] = plane, V2C, R0
                data = dict(points=pts.copy(), gt_boxes=boxes.copy(), gt_names=names.copy(),
                            gt_boxes_mask=np.array([n in CLASSES for n in names], dtype=np.bool_))
                if spec.get("plane", False):
                    data.update(road_plane=plane, calib=calib)
                with Recorder() as rec:
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
                        for s in range(S):
                            if int(out["cand"][b, g, s]) in where and out["cand"][b, g, s] >= 0:
                                out["sample_rot"][b, g, s] = v[where[int(out["cand"][b, g, s])]]
                for axis in spec["flip"]:
                    kind, v = events.pop(0)
                    assert kind == "choice"
                    out["flip_" + axis][b] = v
                (k1, rot), (k2, scale) = events
                assert k1 == "uniform" and k2 == "uniform"
                out["rot"][b], out["scale"][b] = rot, scale
                for g in range(G):
                    for s in range(S):
                        out["sample_valid"][b, g, s] = int(out["cand"][b, g, s] >= 0 and int(out["cand"][b, g, s]) in state["valid"])
                # the collision tests' pairs, group by group, in float64
                wide = lambda bx: bx + np.array([0, 0, 0, *spec.get("collide_extra_width", [0, 0, 0]), 0], np.float32)  # noqa: E731
                existing = wide(boxes.reshape(-1, 7))
                trained = np.array([n in CLASSES for n in names], bool)
                for g in range(G):
                    live = out["cand"][b, g][out["cand"][b, g] >= 0]
                    cb = wide(db["boxes"][live])
                    clear[0] &= pairs_clear(cb, existing)
                    ok = out["sample_valid"][b, g][out["cand"][b, g] >= 0].astype(bool)
                    if len(live):
                        own = c_oracle.pairwise(cb, cb, 1)
                        np.fill_diagonal(own, 0)
                        hit_own = own.max(axis=1) > 0
                        hit_old = c_oracle.pairwise(cb, existing, 1) > 0 if len(existing) else np.zeros((len(live), 0), bool)
                        n_in = len(boxes)
                        hit_untrained = hit_old[:, :n_in][:, ~trained].any(axis=1) if n_in else np.zeros(len(live), bool)
                        hit_rest = np.delete(hit_old, np.nonzero(~trained)[0], axis=1).any(axis=1)
                        stats["only_untrained"] += int((hit_untrained & ~hit_rest & ~hit_own).sum())
                        stats["only_each_other"] += int((hit_own & ~hit_old.any(axis=1)).sum())
                        assert np.array_equal(ok, ~(hit_own | hit_old.any(axis=1))), "the replayed collision test differs from the reference's"
                    existing = np.concatenate([existing, cb[ok]], 0)
                    stats["accepted"] += int(ok.sum())
                    stats["rejected"] += int((~ok).sum())
                # DatasetTemplate.prepare_data between the augmentor and the processor (dataset.py:132-138)
                selected = m["common_utils"].keep_arrays_by_name(data["gt_names"], CLASSES)
                data["gt_boxes"], data["gt_names"] = data["gt_boxes"][selected], data["gt_names"][selected]
                gt_classes = np.array([CLASSES.index(n) + 1 for n in data["gt_names"]], dtype=np.int32)
                data["gt_boxes"] = np.concatenate((data["gt_boxes"], gt_classes.reshape(-1, 1).astype(np.float32)), axis=1)
                clear[0] &= range_clear(data["points"], data["gt_boxes"])
                data = processor.mask_points_and_boxes_outside_range(
                    data_dict=data, config=Cfg(REMOVE_OUTSIDE_BOXES=True, min_num_corners=spec.get("min_num_corners", 1)))
                res_pts.append(np.asarray(data["points"], np.float32))
                res_boxes.append(np.asarray(data["gt_boxes"], np.float32).reshape(-1, 8))
                if not clear[0]:
                    return None
        finally:
            cls_sampler.put_boxes_on_road_planes = staticmethod(inner_plane)
            m["box_utils"].remove_points_in_boxes3d = inner_remove
    T = G * S
    gt_in = np.zeros((B, M, 8), np.float32)
    gt_out = np.zeros((B, M + T, 8), np.float32)
    gt_classes = []
    for b, (pts, boxes, names) in enumerate(frames):
        ids = np.array([CLASSES.index(n) + 1 if n in CLASSES else 0 for n in names], np.float32)
        gt_in[b, :len(boxes), :7], gt_in[b, :len(boxes), 7] = boxes, ids
        gt_out[b, :len(res_boxes[b])] = res_boxes[b]
        gt_classes.append(ids.astype(np.int32))
    spec_checks = spec.get("expect", ())
    if stats["accepted"] == 0 or stats["rejected"] == 0 or stats["carved"] == 0 or any(stats[k] == 0 for k in spec_checks):
        print(f"   seed {seed}: not every situation occurs: {stats}")
        return None
    perm_len = np.array([len(p) for p in perms], np.int32)
    res = dict(
        in_points=np.concatenate([f[0] for f in frames], 0), in_point_offsets=np.cumsum([0] + [len(f[0]) for f in frames]).astype(np.int32),
        in_gt_boxes=gt_in, in_gt_counts=np.array([len(f[1]) for f in frames], np.int32), in_db_points=db["points"],
        in_db_offsets=db["offsets"], in_db_boxes=db["boxes"], in_db_cls=db["cls"], rec_db_difficulty=db["difficulty"], in_cand=out["cand"], in_flip_x=out["flip_x"],
        in_flip_y=out["flip_y"], in_rot=out["rot"], in_scale=out["scale"],
        out_points=np.concatenate(res_pts, 0), out_point_offsets=np.cumsum([0] + [len(p) for p in res_pts]).astype(np.int32),
        out_gt_boxes=gt_out, out_gt_counts=np.array([len(x) for x in res_boxes], np.int32), out_sample_valid=out["sample_valid"],
        rec_perms=np.concatenate(perms).astype(np.int32) if perms else np.zeros(0, np.int32), rec_perm_len=perm_len,
        rec_gt_classes=np.concatenate(gt_classes).astype(np.int32) if gt_classes else np.zeros(0, np.int32))
    if "sample_rot" in spec:
        res["in_sample_rot"] = out["sample_rot"]
    if spec.get("plane", False):
        res.update(rec_plane_abcd=out["plane_abcd"], rec_V2C=out["V2C"], rec_R0=out["R0"],
                   rec_heights=np.concatenate(heights, 0) if heights else np.zeros((0, 6)))
    cfg = dict(remove_extra_width=spec.get("remove_extra_width", [0.0, 0.0, 0.0]), collide_extra_width=spec.get("collide_extra_width"),
               pc_range=PC_RANGE, remove_outside_boxes=True, min_num_corners=spec.get("min_num_corners", 1), apply_scale=True,
               groups=[[CLASSES.index(n) + 1, k] for n, k in groups], limit_whole_scene=spec.get("limit", False),
               removed_difficulty=[-1], min_points={"1": 5}, flip=spec["flip"], plane=spec.get("plane", False), stats=stats)
    return cfg, res


KITTI_GROUPS = [("Car", 15), ("Pedestrian", 10), ("Cyclist", 10)]
CASES = {
    "kitti": dict(C=4, frames=["mixed", "empty", "blocked", "mixed"], groups=KITTI_GROUPS, plane=True, flip=["x"],
                  expect=("only_untrained", "only_each_other")),
    "wide": dict(C=4, frames=["mixed", "mixed", "empty"], groups=KITTI_GROUPS, flip=["x", "y"], collide_extra_width=[0.4, 0.4, 0.0],
                 remove_extra_width=[0.2, 0.2, 0.1], sample_rot=[-0.3, 0.3]),
    "limit": dict(C=4, frames=["cars", "mixed"], groups=[("Car", 6), ("Pedestrian", 4), ("Cyclist", 4)], flip=["x"], limit=True),
    "feat5": dict(C=5, frames=["mixed", "mixed"], groups=KITTI_GROUPS, flip=["x"]),
    "corners8": dict(C=4, frames=["mixed", "mixed"], groups=KITTI_GROUPS, flip=["x"], min_num_corners=8),
}


def main():
    m = load_reference()
    out = {}
    for name, spec in CASES.items():
        for seed in range(300, 700):
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
    path = os.path.join(HERE, "augment_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
