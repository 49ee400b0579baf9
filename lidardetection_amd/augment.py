"""Host side of csrc/augment.hip: train-time augmentation on the device, from "raw clouds + annotations" to "points the voxeliser
sees": GT sampling (pcdet/datasets/augmentor/database_sampler.py), random world flip / rotation / scaling
(pcdet/datasets/augmentor/data_augmentor.py, augmentor_utils.py), the range mask and shuffle_points
(pcdet/datasets/processor/data_processor.py:19-46), for a whole batch in one call (include/lidar_hip.h: lidar_augment).

  GtDatabase       the GT database on the device, built once from host arrays, with the PREPARE filters as host list logic
  DbSampler        sample_with_fixed_number and LIMIT_WHOLE_SCENE on the host: which database objects are candidates
  road_plane_lidar put_boxes_on_road_planes as the 4-vector the kernel evaluates
  TrainAugmentor   draws the per-frame flips, angle and scale on the host, allocates the outputs from torch's caching allocator,
                   launches on the current stream and never synchronises

Multi-frame models (tools/cfgs/livox_models/pv_rcnn_multiframe.yaml): a GtDatabase built with locations / rotations_y and a call given
locations= / rotations_y= go through lidar_augment_mf, which moves every gt's pose in each stacked sweep with its box (the reference's
database_sampler.py:165-177, augmentor_utils.py, data_processor.py:29-32); the result feeds lidardetection_amd/point_head_mf.py.

The kernels draw nothing; every random number comes from a generator (or from arrays) the caller passes."""
import numpy as np
import torch

from . import _lib
from ._lib import LIMITS

MAX_FEATURES, MAX_GROUPS = LIMITS["LIDAR_AUGMENT_MAX_FEATURES"], LIMITS["LIDAR_AUGMENT_MAX_GROUPS"]
MAX_PER_GROUP, MAX_BOXES = LIMITS["LIDAR_AUGMENT_MAX_PER_GROUP"], LIMITS["LIDAR_AUGMENT_MAX_BOXES"]
MAX_FRAMES = LIMITS["LIDAR_AUGMENT_MF_MAX_FRAMES"]


def fakelidar_to_lidar(boxes):
    """box_utils.boxes3d_kitti_fakelidar_to_lidar: [x, y, z bottom, w, l, h, r] -> [x, y, z centre, dx, dy, dz, heading]"""
    b = np.asarray(boxes, np.float32).copy()
    w, l, h, r = b[:, 3:4].copy(), b[:, 4:5].copy(), b[:, 5:6].copy(), b[:, 6:7].copy()
    b[:, 2] += h[:, 0] / 2
    return np.concatenate([b[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1).astype(np.float32)


class GtDatabase:
    """points (P, C) f32: every object's points, object-local as the reference's .bin files store them; offsets (n_obj + 1);
    boxes (n_obj, 7); cls (n_obj) 1-based class ids; difficulty / num_points_in_gt (n_obj) for the PREPARE filters (defaults: 0 and
    the object's point count).  fakelidar=True (DATABASE_WITH_FAKELIDAR): the boxes are converted once, here; the reference moves
    the object points to the unconverted (bottom) centre, so the stored points are lowered by h / 2 to keep that placement.
    locations (n_obj, S, 3), rotations_y (n_obj, S): every object's pose in each of the S stacked sweeps of the multi-frame models,
    in the frame of `boxes` as they are kept here (both or neither; db.S is 0 without them)."""

    def __init__(self, points, offsets, boxes, cls, difficulty=None, num_points_in_gt=None, fakelidar=False, device="cuda",
                 locations=None, rotations_y=None):
        points = np.ascontiguousarray(points, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        boxes = np.ascontiguousarray(boxes, np.float32)
        cls = np.ascontiguousarray(cls, np.int32)
        n = len(cls)
        if points.ndim != 2 or not 3 <= points.shape[1] <= MAX_FEATURES:
            _lib.fail("augment", f"database points must be (P, C) with 3 <= C <= {MAX_FEATURES}, got {points.shape}")
        if boxes.shape != (n, 7) or offsets.shape != (n + 1,):
            _lib.fail("augment", f"database boxes must be ({n}, 7) and offsets ({n + 1},), got {boxes.shape} and {offsets.shape}")
        if n and (offsets[0] != 0 or offsets[-1] != len(points) or np.any(np.diff(offsets) < 0)):
            _lib.fail("augment", "database offsets must ascend from 0 to the number of points")
        if np.any(cls < 1):
            _lib.fail("augment", "database class ids are 1-based")
        if (locations is None) != (rotations_y is None):
            _lib.fail("augment", "database locations and rotations_y come together: one of them is missing")
        self.S = 0
        if locations is not None:
            locations, rotations_y = np.ascontiguousarray(locations, np.float32), np.ascontiguousarray(rotations_y, np.float32)
            if locations.ndim != 3 or locations.shape[0] != n or locations.shape[2] != 3 or rotations_y.shape != locations.shape[:2]:
                _lib.fail("augment", f"database locations must be ({n}, S, 3) and rotations_y ({n}, S), got {locations.shape} and "
                          f"{rotations_y.shape}")
            self.S = int(locations.shape[1])
            if not 1 <= self.S <= MAX_FRAMES:
                _lib.fail("augment", f"1 <= stacked sweeps S <= {MAX_FRAMES}, got database locations {locations.shape}")
        if fakelidar:
            points = points.copy()
            points[:, 2] -= np.repeat(boxes[:, 5] / 2, np.diff(offsets))
            boxes = fakelidar_to_lidar(boxes)
        self.n_obj, self.C = n, int(points.shape[1])
        self.host_offsets = offsets
        self.host_cls = cls
        self.host_boxes = boxes
        self.sizes = np.diff(offsets)
        self.difficulty = np.zeros(n, np.int64) if difficulty is None else np.asarray(difficulty, np.int64)
        self.num_points_in_gt = self.sizes.copy() if num_points_in_gt is None else np.asarray(num_points_in_gt, np.int64)
        dev = torch.device(device)
        self.points = torch.from_numpy(points).to(dev)
        self.offsets = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        self.boxes = torch.from_numpy(boxes).to(dev)
        self.cls = torch.from_numpy(cls).to(dev)
        self.locations = None if locations is None else torch.from_numpy(locations).to(dev)
        self.rotations_y = None if rotations_y is None else torch.from_numpy(rotations_y).to(dev)

    def indices_of_class(self, cls_id, removed_difficulty=(), min_points=0):
        """database indices of one class, in database order, after filter_by_difficulty (database_sampler.py:50-60) and
        filter_by_min_points (:62-77)"""
        keep = self.host_cls == int(cls_id)
        if len(removed_difficulty):
            keep &= ~np.isin(self.difficulty, list(removed_difficulty))
        if min_points > 0:
            keep &= self.num_points_in_gt >= int(min_points)
        return np.nonzero(keep)[0].astype(np.int64)


class DbSampler:
    """sample_with_fixed_number (database_sampler.py:79-96) and LIMIT_WHOLE_SCENE (:195-197) on the host.
    sample_groups: [(class id, sample number), ...] in SAMPLE_GROUPS order; min_points: {class id: n} (filter_by_min_points).
    Per class a pointer and a permutation of its (filtered) database indices, reshuffled with rng.permutation when the pointer has
    run past the end; a batch is sampled frame by frame, group by group, as the reference's workers do for one frame."""

    def __init__(self, db, sample_groups, removed_difficulty=(), min_points=None, limit_whole_scene=False):
        if not 1 <= len(sample_groups) <= MAX_GROUPS:
            _lib.fail("augment", f"1 <= number of sample groups <= {MAX_GROUPS}, got {len(sample_groups)}")
        self.db = db
        self.groups = [(int(c), int(n)) for c, n in sample_groups]
        self.S = max(0, max(n for _, n in self.groups))
        if self.S > MAX_PER_GROUP:
            _lib.fail("augment", f"sample number <= {MAX_PER_GROUP}, got {self.S}")
        self.limit_whole_scene = bool(limit_whole_scene)
        min_points = min_points or {}
        self.pool = [db.indices_of_class(c, removed_difficulty, min_points.get(c, 0)) for c, _ in self.groups]
        self.pointer = [len(p) for p in self.pool]
        self.indices = [np.arange(len(p)) for p in self.pool]

    def sample(self, gt_classes, rng):
        """gt_classes: per frame the host class ids of its annotated objects (any sequence of sequences; only LIMIT_WHOLE_SCENE reads
        them).  rng: np.random.Generator or RandomState.  -> cand (B, G, S) int32 database indices, padded with -1"""
        B, G = len(gt_classes), len(self.groups)
        cand = np.full((B, G, self.S), -1, np.int32)
        for b in range(B):
            for g, (c, num) in enumerate(self.groups):
                if self.limit_whole_scene:
                    num = num - int(np.sum(np.asarray(gt_classes[b]) == c))
                if num <= 0 or not len(self.pool[g]):
                    continue
                if self.pointer[g] >= len(self.pool[g]):
                    self.indices[g] = rng.permutation(len(self.pool[g]))
                    self.pointer[g] = 0
                take = self.indices[g][self.pointer[g]:self.pointer[g] + num]
                self.pointer[g] += num
                cand[b, g, :len(take)] = self.pool[g][take]
        return cand


def road_plane_lidar(plane_abcd, V2C, R0):
    """put_boxes_on_road_planes (database_sampler.py:98-116) is affine in the box centre: the lidar height of the road under
    (x, y, z) is q . [x, y, z, 1].  -> q (4,) float64, from the camera-frame plane [a, b, c, d] and the calibration's Tr_velo2cam
    (3, 4) and R0 (3, 3), in float64 (calibration_kitti.py:50-73)."""
    a, b, c, d = (float(v) for v in plane_abcd)
    V2C, R0 = np.asarray(V2C, np.float64).reshape(3, 4), np.asarray(R0, np.float64).reshape(3, 3)
    to_rect = V2C.T @ R0.T                                      # lidar_to_rect: [x y z 1] @ (V2C.T @ R0.T)
    R0_ext, V2C_ext = np.eye(4), np.eye(4)
    R0_ext[:3, :3] = R0
    V2C_ext[:3, :4] = V2C
    to_lidar = np.linalg.inv((R0_ext @ V2C_ext).T)              # rect_to_lidar: [x y z 1] @ inv((R0_ext @ V2C_ext).T)

    def height(p):
        cam = np.array([*p, 1.0]) @ to_rect
        cam[1] = (-d - a * cam[0] - c * cam[2]) / b
        return (np.array([*cam, 1.0]) @ to_lidar)[2]

    h0 = height([0.0, 0.0, 0.0])
    return np.array([height([1.0, 0, 0]) - h0, height([0, 1.0, 0]) - h0, height([0, 0, 1.0]) - h0, h0], np.float64)


def _uniform(rng, lo, hi, n):
    return np.asarray(rng.uniform(lo, hi, n), np.float64)


class TrainAugmentor:
    """db: GtDatabase; sample_groups: number of groups G of the `cand` it will be given (or the DbSampler's list); pc_range (6);
    world_rot_range [lo, hi] (a number r means [-r, r]); world_scale_range [lo, hi] (scaling is skipped when hi - lo < 1e-3, as
    global_scaling does); flip_axes: subset of "xy"; remove_extra_width (3); collide_extra_width (3) or None
    (REMOVE_SAMPLE_BOXES_EXTRA_WIDTH); sample_rot_range [lo, hi] or None (SAMPLE_ROT_ANGLE); remove_outside_boxes,
    min_num_corners (mask_points_and_boxes_outside_range); frame_points_max: the caller's bound on one frame's input points, used
    for `n_max` when a call has no host offsets."""

    def __init__(self, db, sample_groups, pc_range, world_rot_range=(-0.78539816, 0.78539816), world_scale_range=(0.95, 1.05),
                 flip_axes="x", remove_extra_width=(0.0, 0.0, 0.0), collide_extra_width=None, sample_rot_range=None,
                 remove_outside_boxes=True, min_num_corners=1, frame_points_max=None):
        self.db = db
        self.G = int(sample_groups) if np.isscalar(sample_groups) else len(sample_groups)
        if np.isscalar(world_rot_range):
            world_rot_range = (-float(world_rot_range), float(world_rot_range))
        self.rot_range = tuple(float(v) for v in world_rot_range)
        self.scale_range = tuple(float(v) for v in world_scale_range)
        self.apply_scale = not (self.scale_range[1] - self.scale_range[0] < 1e-3)           # augmentor_utils.py:99
        if any(a not in "xy" for a in flip_axes):
            _lib.fail("augment", f"flip_axes must be a subset of 'xy', got {flip_axes!r}")
        self.flip_axes = "".join(flip_axes)
        self.sample_rot_range = None if sample_rot_range is None else tuple(float(v) for v in sample_rot_range)
        self.pc_range = [float(v) for v in pc_range]
        self._range_h = _lib.host_f32(self.pc_range)
        self._rw_h = _lib.host_f32(remove_extra_width)
        self._cw_h = None if collide_extra_width is None else _lib.host_f32(collide_extra_width)
        self.remove_outside_boxes, self.min_num_corners = bool(remove_outside_boxes), int(min_num_corners)
        self.frame_points_max = frame_points_max
        self._ws = None

    def draw(self, B, S, rng):
        """the per-frame draws of random_flip_along_* (np.random.choice([False, True])), global_rotation and global_scaling
        (np.random.uniform) and SAMPLE_ROT_ANGLE (uniform per candidate) -> dict of host arrays"""
        d = dict(flip_x=np.zeros(B, np.int32), flip_y=np.zeros(B, np.int32))
        for axis in "xy":
            if axis in self.flip_axes:
                d["flip_" + axis] = np.asarray(rng.choice([0, 1], size=B), np.int32)
        d["rot"] = _uniform(rng, *self.rot_range, B).astype(np.float32)
        d["scale"] = _uniform(rng, *self.scale_range, B).astype(np.float32) if self.apply_scale else None
        d["sample_rot"] = None if self.sample_rot_range is None else \
            _uniform(rng, *self.sample_rot_range, (B, self.G, S)).astype(np.float32)
        return d

    def __call__(self, points, point_offsets, gt_boxes, gt_counts, cand, rng=None, planes=None, shuffle=False, flip_x=None,
                 flip_y=None, rot=None, scale=None, sample_rot=None, shuffle_keys=None, host_offsets=None, cap=None, locations=None,
                 rotations_y=None):
        """points (sum N, C) f32, point_offsets (B + 1) i32, gt_boxes (B, M, 8) f32 [box | class id], gt_counts (B) i32: device
        tensors.  cand (B, G, S) int32 HOST array (DbSampler.sample).  rng: the generator the draws come from; flip_x, flip_y, rot,
        scale (B), sample_rot (B, G, S) given explicitly (host arrays) replace their draws.  planes (B, 4): road_plane_lidar per
        frame.  -> dict: points (cap, C), point_offsets (B + 1), gt_boxes (B, M + G * S, 8), gt_counts (B), sample_valid (B, G, S)
        device tensors, n_max (host int: a bound on one output frame's points) — ready for PointPillarKITTI.train_loss(points,
        point_offsets, gt_boxes) with host_offsets=None.  Rows of `points` at and past point_offsets[B] are unspecified.
        locations (B, M, F, 3), rotations_y (B, M, F) f32 device tensors (both or neither; the database must carry poses of the
        same F): the gts' poses in each stacked sweep.  They follow their boxes through every step (lidar_augment_mf) and the dict
        gains locations (B, M + G * S, F, 3) and rotations_y (B, M + G * S, F), zero past gt_counts — what
        point_head_mf.assign_point_targets_mf and enlarged_gt_boxes take."""
        db = self.db
        if points.dim() != 2 or points.dtype != torch.float32:
            _lib.fail("augment", f"points must be float32 (sum N, C), got {points.dtype} {tuple(points.shape)}")
        n_points, C = (int(v) for v in points.shape)
        if C != db.C:
            _lib.fail("augment", f"points have {C} columns, the database {db.C}")
        if point_offsets.dim() != 1 or point_offsets.dtype != torch.int32 or point_offsets.shape[0] < 1:
            _lib.fail("augment", f"point_offsets must be int32 (B + 1,), got {point_offsets.dtype} {tuple(point_offsets.shape)}")
        B = int(point_offsets.shape[0]) - 1
        if gt_boxes.dim() != 3 or gt_boxes.dtype != torch.float32 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 8:
            _lib.fail("augment", f"gt_boxes must be float32 ({B}, M, 8), got {gt_boxes.dtype} {tuple(gt_boxes.shape)}")
        M = int(gt_boxes.shape[1])
        if tuple(gt_counts.shape) != (B,) or gt_counts.dtype != torch.int32:
            _lib.fail("augment", f"gt_counts must be int32 ({B},), got {gt_counts.dtype} {tuple(gt_counts.shape)}")
        if (locations is None) != (rotations_y is None):
            _lib.fail("augment", "locations and rotations_y come together: one of them is missing")
        F = 0
        if locations is not None:
            if (locations.dim() != 4 or tuple(locations.shape[:2]) != (B, M) or locations.shape[3] != 3 or
                    tuple(rotations_y.shape) != tuple(locations.shape[:3]) or locations.dtype != torch.float32 or
                    rotations_y.dtype != torch.float32):
                _lib.fail("augment", f"locations must be float32 ({B}, {M}, S, 3) and rotations_y float32 ({B}, {M}, S), got {locations.dtype} "
                          f"{tuple(locations.shape)} and {rotations_y.dtype} {tuple(rotations_y.shape)}")
            F = int(locations.shape[2])
            if db.S != F or not 1 <= F <= MAX_FRAMES:
                _lib.fail("augment", f"locations {tuple(locations.shape)} need a database with poses of the same 1 <= S <= {MAX_FRAMES}; "
                          f"the database's locations are {None if db.locations is None else tuple(db.locations.shape)}")
        cand = np.asarray(cand)
        if cand.ndim != 3 or cand.shape[0] != B or cand.shape[1] != self.G or not np.issubdtype(cand.dtype, np.integer):
            _lib.fail("augment", f"cand must be an integer ({B}, {self.G}, S) host array, got {cand.dtype} {cand.shape}")
        S = int(cand.shape[2])
        if not (3 <= C <= MAX_FEATURES and 1 <= self.G <= MAX_GROUPS and 0 <= S <= MAX_PER_GROUP and M + self.G * S <= MAX_BOXES):
            _lib.fail("augment", f"supported: 3 <= C <= {MAX_FEATURES}, 1 <= G <= {MAX_GROUPS}, 0 <= S <= {MAX_PER_GROUP}, M + G * S <= {MAX_BOXES}; "
                      f"got C {C}, G {self.G}, S {S}, M {M}")
        if cand.size and (cand.max() >= db.n_obj or cand.min() < -1):
            _lib.fail("augment", f"cand holds an index outside [-1, {db.n_obj})")
        dev = points.device
        # host bounds: every candidate's object counts, valid or not
        per_frame = np.where(cand >= 0, db.sizes[np.maximum(cand, 0)], 0).reshape(B, -1).sum(axis=1) if cand.size else np.zeros(B, np.int64)
        obj_bound = int(per_frame.sum())
        need = n_points + obj_bound
        if cap is None:
            cap = need
        if cap < need:
            _lib.fail("augment", f"cap {cap} is smaller than the bound {need} (input points + the points of every candidate's object)")
        if cap >= 2 ** 31 - 256 * (B + 2):
            _lib.fail("augment", f"cap {cap} does not fit the kernels' int32 row indices")
        if host_offsets is not None:
            n_in = np.diff(np.asarray(host_offsets, np.int64))
            n_max = int((n_in + per_frame).max()) if B else 0
        elif self.frame_points_max is not None:
            n_max = int(self.frame_points_max) + (int(per_frame.max()) if B else 0)
        else:
            n_max = int(cap)
        _lib.require_cuda(points, point_offsets, gt_boxes, gt_counts, locations, rotations_y)
        draws = self.draw(B, S, rng) if rng is not None else {}

        def pick(name, given, shape, dtype, optional=False):
            v = given if given is not None else draws.get(name)
            if v is None:
                if optional:
                    return None
                _lib.fail("augment", f"{name} is neither given nor drawn (pass rng= or {name}=)")
            v = np.ascontiguousarray(v, dtype)
            if v.shape != shape:
                _lib.fail("augment", f"{name} must have shape {shape}, got {v.shape}")
            return v

        fx = pick("flip_x", flip_x, (B,), np.int32)
        fy = pick("flip_y", flip_y, (B,), np.int32)
        rt = pick("rot", rot, (B,), np.float32)
        sc = pick("scale", scale, (B,), np.float32) if self.apply_scale else None
        sr = pick("sample_rot", sample_rot, (B, self.G, S), np.float32, optional=self.sample_rot_range is None)
        pl = None if planes is None else np.ascontiguousarray(planes, np.float32)
        if pl is not None and pl.shape != (B, 4):
            _lib.fail("augment", f"planes must be ({B}, 4), got {pl.shape}")
        rt64 = rt.astype(np.float64)
        rot_cs = np.stack([np.cos(rt64), np.sin(rt64)], axis=1).astype(np.float32)          # in double, rounded once

        def up(a):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)

        d_cand, d_fx, d_fy, d_rot, d_cs, d_sc, d_sr, d_pl = (up(a) for a in (cand.astype(np.int32), fx, fy, rt, rot_cs, sc, sr, pl))
        T = self.G * S
        out = {
            "points": torch.empty((cap, C), dtype=torch.float32, device=dev),
            "point_offsets": torch.empty((B + 1,), dtype=torch.int32, device=dev),
            "gt_boxes": torch.empty((B, M + T, 8), dtype=torch.float32, device=dev),
            "gt_counts": torch.empty((B,), dtype=torch.int32, device=dev),
            "sample_valid": torch.empty((B, self.G, S), dtype=torch.int32, device=dev),
            "n_max": n_max,
        }
        if F:
            out["locations"] = torch.empty((B, M + T, F, 3), dtype=torch.float32, device=dev)
            out["rotations_y"] = torch.empty((B, M + T, F), dtype=torch.float32, device=dev)
        if B == 0:
            out["point_offsets"].zero_()
            return out
        L = _lib.lib()
        ws_bytes = int(L.lidar_augment_workspace_bytes(B, self.G, S, cap))
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != dev:
            self._ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        head = (_lib.ptr(points), _lib.ptr(point_offsets), n_points, C, _lib.ptr(gt_boxes), _lib.ptr(gt_counts), B, M, _lib.ptr(db.points),
                _lib.ptr(db.offsets), _lib.ptr(db.boxes), _lib.ptr(db.cls), db.n_obj, int(db.points.shape[0]), _lib.ptr(d_cand), self.G, S,
                _lib.ptr(d_fx), _lib.ptr(d_fy), _lib.ptr(d_rot), _lib.ptr(d_cs), _lib.ptr(d_sc), _lib.ptr(d_sr), _lib.ptr(d_pl), self._rw_h,
                self._cw_h, self._range_h, int(self.remove_outside_boxes), self.min_num_corners, obj_bound, cap)
        outs = (_lib.ptr(out["points"]), _lib.ptr(out["point_offsets"]), _lib.ptr(out["gt_boxes"]), _lib.ptr(out["gt_counts"]),
                _lib.ptr(out["sample_valid"]))
        tail = (_lib.ptr(self._ws), ws_bytes, _lib.stream())
        if F:
            status = L.lidar_augment_mf(*head, _lib.ptr(locations), _lib.ptr(rotations_y), _lib.ptr(db.locations), _lib.ptr(db.rotations_y),
                                        F, *outs, _lib.ptr(out["locations"]), _lib.ptr(out["rotations_y"]), *tail)
            _lib.check(status, "lidar_augment_mf")
        else:
            _lib.check(L.lidar_augment(*head, *outs, *tail), "lidar_augment")
        if shuffle:
            if shuffle_keys is None:
                if rng is None:
                    _lib.fail("augment", "shuffle=True needs shuffle_keys (cap,) in [0, 1) or rng=")
                shuffle_keys = np.asarray(rng.random(cap), np.float32)
            keys = shuffle_keys if torch.is_tensor(shuffle_keys) else up(np.ascontiguousarray(shuffle_keys, np.float32))
            out["points"] = shuffle_points(out["points"], out["point_offsets"], keys)
        return out


def shuffle_points(points, point_offsets, keys):
    """shuffle_points (data_processor.py:36-46) for a batch: within each frame the rows are reordered by ascending (key, row);
    keys (rows,) f32 in [0, 1).  One device sort, no host read; rows past point_offsets[-1] stay where they are."""
    n = int(points.shape[0])
    if tuple(keys.shape) != (n,) or keys.dtype != torch.float32:
        _lib.fail("augment", f"shuffle keys must be float32 ({n},), got {keys.dtype} {tuple(keys.shape)}")
    rows = torch.arange(n, device=points.device, dtype=torch.int32)
    frame = torch.searchsorted(point_offsets[1:].contiguous(), rows, right=True)            # rows past the end: frame B
    last = int(point_offsets.shape[0]) - 1
    k = torch.where(frame < last, frame.double() + keys.double().clamp(0.0, 1.0 - 2.0 ** -25), (last + rows.double() / max(n, 1)))
    return points[torch.argsort(k, stable=True)]
