"""A float64 numpy restatement of the multi-frame point head (PointHeadSimpleMultiFrame.assign_targets and get_cls_layer_loss with
its analytic gradient) and of the multi-frame union gt boxes (anchor_head_single.py:67-88): the oracle for shapes
tests/golden/point_head_mf_ref.npz does not hold.  tests/test_point_head_mf_host.py pins it to that fixture, i.e. to the reference's
own float64 run (labels and owners exactly, values to 1e-9).  The per-frame targets are tests/_point_head_np.py's, on the
substituted boxes.

Also here, because the generator and both test files need them: the fixture's cases (CASES), the margin of a point to the faces of
every per-frame box (`margins_mf`), and the inputs of the raw-ABI sweep (`sweep_cases`, `sweep_inputs`)."""
import numpy as np

import _point_head_np as ph

EXTRA = ph.EXTRA


def _cfg(weight):
    return dict(CLS_FC=[], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True, TARGET_CONFIG=dict(GT_EXTRA_WIDTH=EXTRA),
                LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=weight)))


# name -> num_class, stack_frame_size, POINT_HEAD config (agnostic3: tools/cfgs/livox_models/pv_rcnn_multiframe.yaml)
CASES = {
    "agnostic3": dict(num_class=1, frames=3, cfg=_cfg(1.0)),
    "classes2": dict(num_class=2, frames=2, cfg=_cfg(1.5)),
    "single": dict(num_class=1, frames=1, cfg=_cfg(1.0)),
}


def substituted(gt_boxes, locations, rotations_y, s):
    """gt_boxes with the centre and heading of frame s (point_head_simple_multiframe.py:45-46)"""
    g = np.array(gt_boxes, copy=True)
    g[..., 0:3] = np.asarray(locations)[:, :, s]
    g[..., 6] = np.asarray(rotations_y)[:, :, s]
    return g


def margins_mf(points, gt_boxes, locations, rotations_y, extra_width):
    """-> (N): _point_head_np.margins over every frame's boxes"""
    S = np.asarray(locations).shape[2]
    return np.min([ph.margins(points, substituted(gt_boxes, locations, rotations_y, s), extra_width) for s in range(S)], axis=0)


def targets(points, gt_boxes, locations, rotations_y, extra_width, num_class):
    """-> labels (N, S) int64, owner (N, S) int32"""
    S = np.asarray(locations).shape[2]
    per = [ph.targets(points, substituted(gt_boxes, locations, rotations_y, s), extra_width, num_class) for s in range(S)]
    return np.stack([t["labels"] for t in per], 1), np.stack([t["owner"] for t in per], 1)


def loss(cls_preds, labels, num_class, weight):
    """cls_preds (N, S * num_class), labels (N, S) -> (cls, npos, d cls / d cls_preds).  The per-point weight is the number of frames
    that do not ignore the point over max(npos, 1); EVERY column carries it, those of an ignoring frame as negative targets."""
    labels = np.asarray(labels)
    N, S = labels.shape
    npos = int((labels > 0).sum())
    w = (labels >= 0).sum(axis=1) / max(npos, 1)
    x = np.asarray(cls_preds, np.float64).reshape(N, S * num_class)
    t = (labels[:, :, None] == np.arange(1, num_class + 1)[None, None]).reshape(N, S * num_class) * 1.0
    v, dv = ph._focal(x, t)
    return float((v * w[:, None]).sum() * weight), npos, dv * w[:, None] * weight


def enlarged(gt_boxes, locations):
    """gt_boxes (B, M, 8), locations (B, M, S, 3) -> (B, M, 8) float64: columns 3, 4 replaced by the x, y extent, in the gt's own
    frame, of the corners of the gt's box placed at each location and turned by the gt's OWN heading"""
    g, loc = np.asarray(gt_boxes, np.float64), np.asarray(locations, np.float64)
    out = g.copy()
    if g.shape[1] == 0:
        return out
    sign = np.array([[1, 1], [1, -1], [-1, -1], [-1, 1]]) / 2.0
    c = g[..., None, 3:5] * sign                                              # (B, M, 4, 2)
    ca, sa = np.cos(g[..., 6])[..., None], np.sin(g[..., 6])[..., None]
    cx, cy = c[..., 0] * ca - c[..., 1] * sa, c[..., 0] * sa + c[..., 1] * ca    # points @ [[cos, sin], [-sin, cos]]
    wx = cx[:, :, None, :] + loc[..., 0:1] - g[..., None, None, 0]             # (B, M, S, 4)
    wy = cy[:, :, None, :] + loc[..., 1:2] - g[..., None, None, 1]
    cb, sb = np.cos(-g[..., 6])[..., None, None], np.sin(-g[..., 6])[..., None, None]
    lx, ly = wx * cb - wy * sb, wx * sb + wy * cb
    out[..., 3] = lx.max(axis=(2, 3)) - lx.min(axis=(2, 3))
    out[..., 4] = ly.max(axis=(2, 3)) - ly.min(axis=(2, 3))
    return out


def moved_poses(r, gt_boxes, frames, shift=0.8, turn=0.3):
    """poses for `frames` stacked sweeps: frame 0 is the gt's own pose, later frames drift and turn; padding rows stay zero"""
    gt = np.asarray(gt_boxes, np.float32)
    B, M = gt.shape[:2]
    loc = np.repeat(gt[:, :, None, 0:3], frames, axis=2)
    rot = np.repeat(gt[:, :, None, 6], frames, axis=2)
    step = np.cumsum(r.normal(0, 1, (B, M, frames, 3)) * np.float32([shift, shift, 0.05]), axis=2)
    dturn = np.cumsum(r.normal(0, turn, (B, M, frames)), axis=2)
    step[:, :, 0], dturn[:, :, 0] = 0, 0
    real = (gt[..., 3] > 0)[..., None]
    loc = np.where(real[..., None], loc + step, 0).astype(np.float32)
    rot = np.where(real, rot + dturn, 0).astype(np.float32)
    return loc, rot


# ------------------------------------------------------------------------------------------------ the raw-ABI sweep's inputs
SWEEP_N, SWEEP_M, SWEEP_S, SWEEP_C, SWEEP_B = (0, 1, 255, 256, 257, 1000), (0, 1, 128), (1, 3, 8), (1, 4), (1, 64)
SWEEP_POS = ("mixed", "all", "none", "ignored")


def sweep_cases():
    """every N with every M; S, num_class, batch and the mode rotate so that each of their values meets every N and every M
    -> (N, M, S, num_class, batch, positives, seed)"""
    for i, N in enumerate(SWEEP_N):
        for j, M in enumerate(SWEEP_M):
            yield (N, M, SWEEP_S[(i + j) % 3], SWEEP_C[(i + j // 2) % 2], SWEEP_B[(i // 2 + j) % 2], SWEEP_POS[(i + 2 * j) % 4], 9000 + 4 * i + j)
    for k, (S, C, B, pos) in enumerate(((8, 4, 64, "mixed"), (8, 1, 1, "ignored"), (3, 4, 1, "all"), (1, 4, 64, "none"), (3, 1, 64, "mixed"))):
        yield 1000, 128, S, C, B, pos, 9100 + k


def sweep_inputs(seed, N, M, S, num_class, B, positives):
    """-> points (N, 4) f32 in shuffled frame order, gt_boxes (B, M, 8), locations (B, M, S, 3), rotations_y (B, M, S) f32.  With
    B == 64 only some batch entries have points.  positives: "mixed" (half of the points around a gt's pose in a random frame,
    half anywhere), "all" (every point inside the first gt of its entry in every frame: that gt does not move), "none" (every
    point far above the boxes), "ignored" (every point in the shell of the first gt, which does not move, and in no box).  Points
    within 1e-4 of a face of any per-frame box or enlarged box are redrawn."""
    r = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    if M:
        gt[..., 0:2] = r.uniform(-20, 20, (B, M, 2))
        gt[..., 2] = r.uniform(-1.5, 0.5, (B, M))
        gt[..., 3:6] = np.asarray(ph.MEAN_SIZE, np.float32)[r.integers(0, 3, (B, M))] * r.uniform(0.8, 1.2, (B, M, 3))
        gt[..., 6] = r.uniform(-7, 7, (B, M))
        gt[..., 7] = r.integers(1, num_class + 1, (B, M))
        gt[r.uniform(size=(B, M)) < 0.2] = 0                  # padding rows, anywhere in the list
        gt[:, 0] = np.where(gt[:, 0, 3:4] > 0, gt[:, 0], np.float32([1, 2, -0.5, 3.9, 1.6, 1.5, 0.3, 1]))      # the first gt is real
    loc, rot = moved_poses(r, gt, S)
    if positives in ("all", "ignored") and M:
        loc[:, 0], rot[:, 0] = gt[:, 0, None, 0:3], gt[:, 0, None, 6]
        if positives == "ignored":                            # nothing else anywhere near: the other rows go far away
            gt[:, 1:, 0:2] += 500
            loc[:, 1:, :, 0:2] += 500
            loc[:, 1:][gt[:, 1:, 3] == 0] = 0                 # padding rows keep zero poses
            gt[:, 1:][gt[:, 1:, 3] == 0] = 0
    entries = np.arange(B) if B == 1 else r.choice(B, 5, replace=False)
    pts = np.zeros((N, 4), np.float32)
    todo = np.arange(N)
    while len(todo):
        n = len(todo)
        bs = entries[r.integers(0, len(entries), n)]
        xyz = np.stack([r.uniform(-22, 22, n), r.uniform(-22, 22, n), r.uniform(-2.5, 1.5, n)], 1)
        if M and positives in ("all", "ignored"):
            g = gt[bs, 0].astype(np.float64)
            l3 = r.uniform(-0.45, 0.45, (n, 3)) * g[:, 3:6]
            if positives == "ignored":                        # 5 to 8 cm beyond the +x face (GT_EXTRA_WIDTH / 2 is 10 cm)
                l3[:, 0] = g[:, 3] / 2 + r.uniform(0.05, 0.08, n)
            c, s = np.cos(g[:, 6]), np.sin(g[:, 6])
            xyz = np.stack([l3[:, 0] * c - l3[:, 1] * s, l3[:, 0] * s + l3[:, 1] * c, l3[:, 2]], 1) + g[:, 0:3]
        elif M and positives == "mixed":
            near = r.uniform(size=n) < 0.5
            k, s = r.integers(0, M, n), r.integers(0, S, n)
            around = loc[bs, k, s] + r.normal(0, 1, (n, 3)) * np.maximum(gt[bs, k, 3:6], 0.3) * 0.6
            xyz[near] = around[near]
        if positives == "none":
            xyz[:, 2] += 50.0
        pts[todo, 0], pts[todo, 1:4] = bs, xyz
        todo = todo[margins_mf(pts[todo], gt, loc, rot, EXTRA) < 1e-4]
    return pts, gt, loc, rot
