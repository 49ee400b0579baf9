"""Plain-numpy restatement of the second-stage target assignment (ProposalTargetLayer + RoIHeadTemplate.assign_targets) under the
randomness contract of include/lidar_hip.h, shared by tests/test_proposal_target_host.py and tests/test_gpu_proposal_target.py.

It is trusted as an oracle for random sweeps only because the host test shows that it reproduces every case of
tests/golden/proposal_target_ref.npz (written by the reference itself): index outputs exactly, floats to 1e-6 of scale.

Everything is float32 arithmetic in the reference's op order.  `overlap_fn(a, b)` is the rotated BEV overlap area of (N, 7) and
(M, 7) boxes; `sample_frame` can instead be fed a max_overlaps / gt_assignment pair computed elsewhere (the GPU's own), which
takes threshold noise out of a comparison of the sampling and labelling logic."""
import json
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposal_target_ref.npz")
CASES = ["pv", "pointrcnn", "parta2", "noclass", "enlarged", "vel"]
PV_RCNN_CFG = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
                   CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)


def load_case(name):
    """-> (cfg dict, inputs dict, expected dict) of numpy arrays"""
    z = np.load(GOLDEN)
    cfg = json.loads(str(z[f"{name}_cfg"]))
    pre = f"{name}_in_"
    inputs = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    pre = f"{name}_out_"
    exp = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return cfg, inputs, exp


def kept_rows(gt):
    """k + 1 of `k = M - 1; while k > 0 and gt[k].sum() == 0: k -= 1`, the row summed left to right in float32"""
    k = gt.shape[0] - 1
    while k > 0:
        s = F(0)
        for v in gt[k]:
            s = F(s + F(v))
        if s != 0:
            break
        k -= 1
    return k + 1


def iou3d(a, b, overlap_fn):
    """boxes_iou3d_gpu: BEV overlap x z overlap / clamp(vol_a + vol_b - overlap, 1e-6)"""
    a, b = a.astype(F), b.astype(F)
    bev = overlap_fn(a[:, :7], b[:, :7]).astype(F)
    a_hi, a_lo = (a[:, 2] + a[:, 5] / F(2))[:, None], (a[:, 2] - a[:, 5] / F(2))[:, None]
    b_hi, b_lo = (b[:, 2] + b[:, 5] / F(2))[None, :], (b[:, 2] - b[:, 5] / F(2))[None, :]
    oh = np.maximum(np.minimum(a_hi, b_hi) - np.maximum(a_lo, b_lo), F(0))
    o3 = bev * oh
    vol_a, vol_b = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None, :]
    return o3 / np.maximum(vol_a + vol_b - o3, F(1e-6))


def max_overlaps(rois, roi_labels, gt, by_class, overlap_fn):
    """rois (R, D), gt (K, D + 1) kept rows -> max_overlaps (R,) f32, gt_assignment (R,) int"""
    R = rois.shape[0]
    if not by_class:
        iou = iou3d(rois[:, :7], gt[:, :7], overlap_fn)
        return iou.max(axis=1), iou.argmax(axis=1)
    ov, asg = np.zeros(R, F), np.zeros(R, np.int64)
    gl = gt[:, -1].astype(np.int64)
    for c in range(int(gl.min()), int(gl.max()) + 1):
        rm, gm = roi_labels == c, gl == c
        if rm.sum() > 0 and gm.sum() > 0:
            iou = iou3d(rois[rm][:, :7], gt[gm][:, :7], overlap_fn)
            ov[rm] = iou.max(axis=1)
            asg[rm] = np.nonzero(gm)[0][iou.argmax(axis=1)]
    return ov, asg


def pick(draws, n):
    """with-replacement picks: min(floor(draw * n), n - 1), the product in float32"""
    return np.minimum(np.floor(draws.astype(F) * F(n)).astype(np.int64), n - 1)


def subsample(ov, cfg, fg_keys, draws):
    """-> sampled roi indices (P,) or None for a frame with neither fg nor bg"""
    P = cfg["ROI_PER_IMAGE"]
    fg_per_image = int(np.round(cfg["FG_RATIO"] * P))
    fg_thresh = F(min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"]))
    lo, reg = F(cfg["CLS_BG_THRESH_LO"]), F(cfg["REG_FG_THRESH"])
    fg = np.nonzero(ov >= fg_thresh)[0]
    easy = np.nonzero(ov < lo)[0]
    hard = np.nonzero((ov < reg) & (ov >= lo))[0]
    n_bg = len(hard) + len(easy)
    if len(fg) == 0 and n_bg == 0:
        return None
    if len(fg) > 0 and n_bg > 0:
        n_fg = min(fg_per_image, len(fg))
        order = np.lexsort((fg, fg_keys[fg].astype(F) + F(0)))       # by (key, roi index)
        out = list(fg[order[:n_fg]])
    elif len(fg) > 0:
        return fg[pick(draws[:P], len(fg))]
    else:
        n_fg, out = 0, []
    n_bg_slots = P - n_fg
    if len(hard) > 0 and len(easy) > 0:
        n_hard = min(int(n_bg_slots * cfg["HARD_BG_RATIO"]), len(hard))
    elif len(hard) > 0:
        n_hard = n_bg_slots
    else:
        n_hard = 0
    if n_hard > 0:
        out += list(hard[pick(draws[n_fg:n_fg + n_hard], len(hard))])
    if n_bg_slots - n_hard > 0:
        out += list(easy[pick(draws[n_fg + n_hard:P], len(easy))])
    return np.array(out, np.int64)


def py_mod(x, m):
    r = np.fmod(x.astype(F), F(m))
    return np.where((r != 0) & (r < 0), r + F(m), r).astype(F)


def canonical(rois, gt_of_rois):
    """assign_targets: rois (P, D), gt_of_rois (P, D + 1) -> (P, D + 1) in the roi's frame, heading folded into [-pi/2, pi/2]"""
    two_pi, pi = F(2 * np.pi), F(np.pi)
    out = gt_of_rois.astype(F).copy()
    ry = py_mod(rois[:, 6], two_pi)
    x, y, z = out[:, 0] - rois[:, 0], out[:, 1] - rois[:, 1], out[:, 2] - rois[:, 2]
    h = out[:, 6] - ry
    c, s = np.cos(ry.astype(np.float64)).astype(F), np.sin(ry.astype(np.float64)).astype(F)
    out[:, 0], out[:, 1], out[:, 2] = x * c + y * s, y * c - x * s, z
    h = py_mod(h, two_pi)
    opp = (h > F(np.pi * 0.5)) & (h < F(np.pi * 1.5))
    h = np.where(opp, py_mod(h + pi, two_pi), h)
    h = np.where(h > pi, h - two_pi, h).astype(F)
    out[:, 6] = np.clip(h, F(-np.pi / 2), F(np.pi / 2))
    return out


def labels_of(ov, cfg):
    """-> reg_valid_mask (int64), rcnn_cls_labels (int64 for 'cls', float32 for 'roi_iou')"""
    ov = ov.astype(F)
    reg_valid = (ov > F(cfg["REG_FG_THRESH"])).astype(np.int64)
    fg_t, bg_t = F(cfg["CLS_FG_THRESH"]), F(cfg["CLS_BG_THRESH"])
    if cfg["CLS_SCORE_TYPE"] == "cls":
        lab = (ov > fg_t).astype(np.int64)
        lab[(ov > bg_t) & (ov < fg_t)] = -1
        return reg_valid, lab
    fg, bg = ov > fg_t, ov < bg_t
    lab = fg.astype(F)
    mid = ~fg & ~bg
    lab[mid] = (ov[mid] - bg_t) / F(cfg["CLS_FG_THRESH"] - cfg["CLS_BG_THRESH"])
    return reg_valid, lab


def sample_frame(rois, scores, labels, gt_rows, ov, asg, cfg, fg_keys, draws):
    """one frame from its max_overlaps / gt_assignment; gt_rows: the rows gt_of_rois is gathered from"""
    P, D = cfg["ROI_PER_IMAGE"], rois.shape[1]
    idx = subsample(ov, cfg, fg_keys, draws)
    if idx is None:
        z = lambda *s, dt=F: np.zeros(s, dt)   # noqa: E731
        lab_dt = np.int64 if cfg["CLS_SCORE_TYPE"] == "cls" else F
        return dict(rois=z(P, D), gt_of_rois=z(P, D + 1), gt_of_rois_src=z(P, D + 1), gt_iou_of_rois=z(P), roi_scores=z(P),
                    roi_labels=z(P, dt=np.int64), reg_valid_mask=z(P, dt=np.int64), rcnn_cls_labels=z(P, dt=lab_dt),
                    sampled_inds=z(P, dt=np.int64), frame_status=1)
    src = gt_rows[asg[idx]].astype(F)
    reg_valid, cls_labels = labels_of(ov[idx], cfg)
    return dict(rois=rois[idx], gt_of_rois=canonical(rois[idx], src), gt_of_rois_src=src, gt_iou_of_rois=ov[idx].astype(F),
                roi_scores=scores[idx], roi_labels=labels[idx].astype(np.int64), reg_valid_mask=reg_valid,
                rcnn_cls_labels=cls_labels, sampled_inds=idx, frame_status=0)


def restate(cfg, rois, roi_scores, roi_labels, gt_boxes, fg_keys, draws, gt_boxes_enlarged=None, overlap_fn=None, overlaps=None):
    """the whole batch -> dict of stacked arrays (+ max_overlaps, gt_assignment).  overlaps: None (computed with overlap_fn) or a
    (max_overlaps (B, R), gt_assignment (B, R)) pair to sample and label from."""
    frames = []
    src_all = gt_boxes if gt_boxes_enlarged is None else gt_boxes_enlarged
    for b in range(rois.shape[0]):
        k = kept_rows(src_all[b])
        if overlaps is None:
            ov, asg = max_overlaps(rois[b], roi_labels[b], src_all[b][:k], cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False), overlap_fn)
        else:
            ov, asg = overlaps[0][b].astype(F), overlaps[1][b].astype(np.int64)
        f = sample_frame(rois[b], roi_scores[b], roi_labels[b], gt_boxes[b][:k], ov, asg, cfg, fg_keys[b], draws[b])
        f["max_overlaps"], f["gt_assignment"], f["kept"] = ov, asg, k
        frames.append(f)
    return {key: np.stack([np.asarray(f[key]) for f in frames]) for key in frames[0]}
