"""A float64 numpy restatement of the point heads' targets and loss (PointHeadTemplate.assign_stack_targets with
set_ignore_flag=True, get_cls_layer_loss, get_box_layer_loss, get_part_layer_loss; PointResidualCoder.encode_torch) with analytic
gradients: the oracle for shapes tests/golden/point_head_ref.npz does not hold.  tests/test_point_head_host.py pins it to that
fixture, i.e. to the reference's own float64 run (labels and owners exactly, values to 1e-9).

The part term is BCE in its stable logits form, which equals the reference's binary_cross_entropy(sigmoid(x), t) in float64 wherever
its -100 log clamp does not engage (|x| < 36 or so).

Also here, because the generator and both test files need them: the fixture's cases with their configs (CASES), the margin of a
point to the faces of the boxes of its frame (`margins`), and the inputs of the raw-ABI sweep (`sweep_inputs`)."""
import numpy as np

MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
EXTRA = [0.2, 0.2, 0.2]
# name -> head class, num_class, model_cfg (plain dicts; the tests wrap them), predictions the head makes
CASES = {
    "pv": dict(head="PointHeadSimple", num_class=1, box=False, part=False,
               cfg=dict(CLS_FC=[], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True, TARGET_CONFIG=dict(GT_EXTRA_WIDTH=EXTRA),
                        LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0)))),
    "pointrcnn": dict(head="PointHeadBox", num_class=3, box=True, part=False,
                      cfg=dict(CLS_FC=[], REG_FC=[], CLASS_AGNOSTIC=False, USE_POINT_FEATURES_BEFORE_FUSION=False,
                               TARGET_CONFIG=dict(GT_EXTRA_WIDTH=EXTRA, BOX_CODER="PointResidualCoder",
                                                  BOX_CODER_CONFIG=dict(use_mean_size=True, mean_size=MEAN_SIZE)),
                               LOSS_CONFIG=dict(LOSS_REG="WeightedSmoothL1Loss",
                                                LOSS_WEIGHTS=dict(point_cls_weight=1.0, point_box_weight=1.0,
                                                                  code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])))),
    "parta2": dict(head="PointIntraPartOffsetHead", num_class=3, box=False, part=True,
                   cfg=dict(CLS_FC=[], PART_FC=[], CLASS_AGNOSTIC=True, TARGET_CONFIG=dict(GT_EXTRA_WIDTH=EXTRA),
                            LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0, point_part_weight=1.0)))),
    "parta2_box": dict(head="PointIntraPartOffsetHead", num_class=3, box=True, part=True,
                       cfg=dict(CLS_FC=[], PART_FC=[], REG_FC=[], CLASS_AGNOSTIC=True,
                                TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.3, 0.1, 0.2], BOX_CODER="PointResidualCoder",
                                                   BOX_CODER_CONFIG=dict(use_mean_size=False)),
                                LOSS_CONFIG=dict(LOSS_REG="WeightedSmoothL1Loss",
                                                 LOSS_WEIGHTS=dict(point_cls_weight=2.0, point_box_weight=0.5, point_part_weight=1.5,
                                                                   code_weights=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 1.25])))),
}


def case_spec_args(name):
    """-> (extra_width, num_class, mean_size or None, weights (3), code_weights (8)) of a fixture case"""
    c = CASES[name]
    t, lw = c["cfg"]["TARGET_CONFIG"], c["cfg"]["LOSS_CONFIG"]["LOSS_WEIGHTS"]
    mean = t.get("BOX_CODER_CONFIG", {}).get("mean_size") if t.get("BOX_CODER_CONFIG", {}).get("use_mean_size") else None
    return (t["GT_EXTRA_WIDTH"], c["num_class"], mean,
            [lw["point_cls_weight"], lw.get("point_box_weight", 0.0), lw.get("point_part_weight", 0.0)],
            lw.get("code_weights", [1.0] * 8))


def _local(p, g):
    """points (n, 3) against the boxes (M, 7+) of their frame -> lx, ly, dz (n, M) in float64"""
    d = p[:, None, :] - g[None, :, 0:3]
    ca, sa = np.cos(-g[:, 6])[None], np.sin(-g[:, 6])[None]
    return d[..., 0] * ca + d[..., 1] * (-sa), d[..., 0] * sa + d[..., 1] * ca, d[..., 2]


def _signed(lx, ly, dz, dims):
    """per axis |local| - threshold (check_pt_in_box3d: x and y strictly below half + MARGIN 1e-5, z at most half)"""
    m = float(np.float32(1e-5))
    return np.abs(lx) - (dims[None, :, 0] / 2 + m), np.abs(ly) - (dims[None, :, 1] / 2 + m), np.abs(dz) - dims[None, :, 2] / 2


def _inside(lx, ly, dz, dims):
    sx, sy, sz = _signed(lx, ly, dz, dims)
    return (sz <= 0) & (sx < 0) & (sy < 0)


def margins(points, gt_boxes, extra_width):
    """-> (N): how far each point is from changing sides of the nearest face of any box or enlarged box of its frame (the distance
    of max_axis(|local| - threshold) from 0); inf for rows outside every frame or frames without rows"""
    points, gt = np.asarray(points, np.float64), np.asarray(gt_boxes, np.float64)
    out = np.full(len(points), np.inf)
    for b in range(gt.shape[0]):
        idx = np.nonzero(points[:, 0] == b)[0]
        if not len(idx) or gt.shape[1] == 0:
            continue
        lx, ly, dz = _local(points[idx, 1:4], gt[b])
        for dims in (gt[b][:, 3:6], gt[b][:, 3:6] + np.asarray(extra_width, np.float64)):
            s = np.maximum(np.maximum(*_signed(lx, ly, dz, dims)[:2]), _signed(lx, ly, dz, dims)[2])
            out[idx] = np.minimum(out[idx], np.abs(s).min(axis=1))
    return out


def targets(points, gt_boxes, extra_width, num_class, mean_size=None, ret_box=False, ret_part=False):
    """-> dict(labels (N) int64, owner (N) int32, box (N, 8) float64 or None, part (N, 3) float64 or None)"""
    points, gt = np.asarray(points, np.float64), np.asarray(gt_boxes, np.float64)
    N, (B, M) = len(points), gt.shape[:2]
    labels, owner = np.zeros(N, np.int64), np.full(N, -1, np.int32)
    box = np.zeros((N, 8)) if ret_box else None
    part = np.zeros((N, 3)) if ret_part else None
    mean = None if mean_size is None else np.asarray(mean_size, np.float64)
    for b in range(B):
        idx = np.nonzero(points[:, 0] == b)[0]
        if not len(idx) or M == 0:
            continue
        p, g = points[idx, 1:4], gt[b]
        lx, ly, dz = _local(p, g)
        ins = _inside(lx, ly, dz, g[:, 3:6])
        ext = _inside(lx, ly, dz, g[:, 3:6] + np.asarray(extra_width, np.float64)).any(axis=1)
        fg = ins.any(axis=1)
        own = np.where(fg, ins.argmax(axis=1), -1)
        lab = np.where(fg ^ ext, -1, 0)
        row = g[own[fg]]
        cls = row[:, 7].astype(np.int64)
        lab[fg] = 1 if num_class == 1 else cls
        labels[idx], owner[idx] = lab, own
        fi = idx[fg]
        if ret_box and len(fi):
            dg = np.maximum(row[:, 3:6], 1e-5)
            with np.errstate(all="ignore"):
                if mean is not None:
                    a = mean[cls - 1]
                    diag = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)
                    ctr = (row[:, 0:3] - p[fg]) / np.stack([diag, diag, a[:, 2]], 1)
                    size = np.log(dg / a)
                else:
                    ctr, size = row[:, 0:3] - p[fg], np.log(dg)
            box[fi] = np.concatenate([ctr, size, np.cos(row[:, 6:7]), np.sin(row[:, 6:7])], 1)
        if ret_part and len(fi):
            k = own[fg]
            local = np.stack([lx[fg, k], ly[fg, k], dz[fg, k]], 1)
            # dims unclamped, unless box labels were made first: encode_torch clamps the rows it is handed IN PLACE at 1e-5
            dims = np.maximum(row[:, 3:6], 1e-5) if ret_box else row[:, 3:6]
            with np.errstate(all="ignore"):
                part[fi] = local / dims + 0.5
    return dict(labels=labels, owner=owner, box=box, part=part)


def _focal(x, t):
    """SigmoidFocalClassificationLoss element (alpha 0.25, gamma 2) and its derivative as autograd forms it"""
    p = 1.0 / (1.0 + np.exp(-x))
    aw = t * 0.25 + (1 - t) * 0.75
    pt = t * (1 - p) + (1 - t) * p
    fw = aw * pt * pt
    e = np.exp(-np.abs(x))
    bce = np.maximum(x, 0) - x * t + np.log1p(e)
    dfw = aw * 2 * pt * (1 - 2 * t) * (1 - p) * p
    dbce = (x >= 0) * 1.0 - t - e / (1 + e) * np.sign(x)
    return fw * bce, dfw * bce + fw * dbce


def loss(cls_preds, box_preds, part_preds, labels, box_labels, part_labels, num_class, weights, code_weights):
    """-> (losses (3) weighted, npos, (d cls / d cls_preds, d box / d box_preds, d part / d part_preds)); a term whose prediction is
    None is 0 with gradient None"""
    labels = np.asarray(labels).reshape(-1)
    pos = labels > 0
    npos = int(pos.sum())
    norm = max(npos, 1)
    out, grads = [0.0, 0.0, 0.0], [None, None, None]
    if cls_preds is not None:
        x = np.asarray(cls_preds, np.float64).reshape(-1, num_class)
        t = (labels[:, None] == np.arange(1, num_class + 1)[None]) * 1.0
        v, dv = _focal(x, t)
        w = (labels >= 0)[:, None] * (weights[0] / norm)
        out[0], grads[0] = float((v * w).sum()), dv * w
    if box_preds is not None:
        x, t = np.asarray(box_preds, np.float64), np.asarray(box_labels, np.float64)
        cw = np.asarray(code_weights, np.float64)[None]
        d = np.where(np.isnan(t), 0.0, (x - np.where(np.isnan(t), x, t)) * cw)
        n, beta = np.abs(d), 1.0 / 9.0
        v = np.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
        dv = np.where(np.isnan(t), 0.0, np.where(n < beta, n / beta, 1.0) * np.sign(d) * cw)
        w = pos[:, None] * (weights[1] / norm)
        out[1], grads[1] = float((v * w)[pos].sum()), dv * w
    if part_preds is not None:
        x, t = np.asarray(part_preds, np.float64), np.asarray(part_labels, np.float64)
        t = np.where(pos[:, None], t, 0.0)                    # the labels of the other rows carry no weight (and may be NaN)
        e = np.exp(-np.abs(x))
        v = np.maximum(x, 0) - x * t + np.log1p(e)
        dv = np.where(x >= 0, 1 / (1 + e), e / (1 + e)) - t
        w = pos[:, None] * (weights[2] / (3 * norm))
        out[2], grads[2] = float((v * w).sum()), dv * w
    return np.array(out), npos, grads


# ------------------------------------------------------------------------------------------------ the raw-ABI sweep's inputs
SWEEP_N, SWEEP_M, SWEEP_B, SWEEP_C = (1, 63, 64, 255, 256, 257, 4097), (0, 1, 7, 65), (1, 3), (1, 3)
SWEEP_POS = ("none", "one", "all", "mixed")


def sweep_cases():
    """every N with every M; the other axes rotate so that every pair of values of two different axes occurs (a host test checks
    that), then every N with every M > 0 in the mixed mode -> (N, M, B, num_class, positives, seed)"""
    for i, N in enumerate(SWEEP_N):
        for j, M in enumerate(SWEEP_M):
            yield N, M, SWEEP_B[(i + j // 2) % 2], SWEEP_C[(i + j + i // 2) % 2], SWEEP_POS[(i + j + i // 4) % 4], 7000 + 4 * i + j
    # and the mixed mode, the one in which rows behind row 0, shells and padding rows decide, at every N with every M > 0
    for i, N in enumerate(SWEEP_N):
        for j, M in enumerate(SWEEP_M):
            if M and SWEEP_POS[(i + j + i // 4) % 4] != "mixed":
                yield N, M, SWEEP_B[(i + j) % 2], SWEEP_C[(i // 2 + j) % 2], "mixed", 7100 + 4 * i + j


def sweep_inputs(seed, N, M, B, num_class, positives):
    """-> (points (N, 4) f32 in shuffled frame order, gt_boxes (B, M, 8) f32 with about a fifth of the rows zero padding, dropped
    fraction).  positives: "none" (every point far above the boxes), "one" (the same, and one point at a gt centre when there is a gt), "all"
    (every point inside the first gt of its frame when there is one), "mixed" (half of the points around a random row of their
    frame - inside it, in its shell only or just outside, padding rows at the origin included -, half anywhere; with N >= 64 and a
    padding row somewhere, row 0 is a point exactly at the origin of a frame that has one).  Points whose margin to any face is
    below 1e-4 are redrawn (the planted origin point is exempt: every operand of its test is exactly 0); the fraction of draws
    dropped that way is returned."""
    r = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    if M:
        gt[..., 0:2] = r.uniform(-20, 20, (B, M, 2))
        gt[..., 2] = r.uniform(-1.5, 0.5, (B, M))
        gt[..., 3:6] = np.asarray(MEAN_SIZE, np.float32)[r.integers(0, 3, (B, M))] * r.uniform(0.8, 1.2, (B, M, 3))
        gt[..., 6] = r.uniform(-7, 7, (B, M))
        gt[..., 7] = r.integers(1, num_class + 1, (B, M))
        gt[r.uniform(size=(B, M)) < 0.2] = 0                  # padding rows, anywhere in the list
        gt[:, 0] = np.where(gt[:, 0, 3:4] > 0, gt[:, 0], np.float32([1, 2, -0.5, 3.9, 1.6, 1.5, 0.3, 1]))      # frame's first gt is real
    extra = np.asarray(EXTRA, np.float64)
    pts = np.zeros((N, 4), np.float32)
    todo, drawn, dropped = np.arange(N), 0, 0
    while len(todo):
        n = len(todo)
        bs = r.integers(0, B, n)
        if positives == "all" and M:
            g = gt[bs, 0]
            loc = r.uniform(-0.45, 0.45, (n, 3)) * g[:, 3:6]
            c, s = np.cos(g[:, 6]), np.sin(g[:, 6])
            xyz = np.stack([loc[:, 0] * c - loc[:, 1] * s, loc[:, 0] * s + loc[:, 1] * c, loc[:, 2]], 1) + g[:, 0:3]
        else:
            # half near a gt (inside, in the shell or just outside), half anywhere
            xyz = np.stack([r.uniform(-22, 22, n), r.uniform(-22, 22, n), r.uniform(-2.5, 1.5, n)], 1)
            if M:
                near = r.uniform(size=n) < 0.5
                g = gt[bs, r.integers(0, M, n)]
                xyz[near] = (g[:, 0:3] + r.normal(0, 1, (n, 3)) * np.maximum(g[:, 3:6], 0.3) * 0.6)[near]
            if positives in ("none", "one"):
                xyz[:, 2] += 50.0
        pts[todo, 0], pts[todo, 1:4] = bs, xyz
        ok = margins(pts[todo], gt, extra) >= 1e-4
        drawn, dropped = drawn + n, dropped + int((~ok).sum())
        todo = todo[~ok]
    if positives == "one" and M:
        pts[N // 2, 0], pts[N // 2, 1:4] = B - 1, gt[B - 1, 0, 0:3]
    if positives == "mixed" and N >= 64 and M:
        padded = np.nonzero((gt[..., 3] == 0).any(axis=1))[0]
        if len(padded):
            pts[0] = [padded[0], 0.0, 0.0, 0.0]
    return pts, gt, dropped / max(drawn, 1)
