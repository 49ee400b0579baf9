"""numpy restatement of ATSS anchor target assignment with THIS repo's tie rules (csrc/atss_assign.hip); test
infrastructure, written for this repo.  The rotated IoU is an input (`iou_fn`), so the same restatement runs on recorded
reference IoUs, on the library's host IoU, or on the device's boxes_iou_bev / boxes_iou3d_gpu.

Tie rules: top-k by ascending (distance, anchor index); per anchor the largest IoU, then the lowest gt; per gt the argmax over
the set at the lowest anchor index; several gts forcing one anchor: the highest gt wins.

fp32 throughout, in the kernel's operation order: the trim sums a row left to right, the distance is
sqrt((dx * dx + dy * dy) + dz * dz), the candidates' mean and unbiased std are sequential sums."""
import json
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atss_assign_ref.npz")
CASES = ["kitti", "kitti_k2", "nus", "kitti_3d"]


def load_case(name):
    """-> meta, the reference's anchor tensors, the same flattened in output order, gt, {(frame, set): the IoU matrix the reference
    saw}, (labels, targets, weights) of the reference"""
    z = np.load(GOLDEN)
    meta = json.loads(str(z[f"{name}_meta"]))
    anchors = [z[f"{name}_anchors_{k}"] for k in range(meta["num_anchors"])]
    flat = [np.ascontiguousarray(a.transpose(3, 4, 0, 1, 2, 5) if meta["use_multihead"] else a).reshape(-1, a.shape[-1])
            for a in anchors]
    ious = {(b, k): z[f"{name}_iou_{b}_{k}"] for b in range(z[f"{name}_gt"].shape[0]) for k in range(len(anchors))}
    return meta, anchors, flat, z[f"{name}_gt"], ious, (z[f"{name}_labels"], z[f"{name}_targets"], z[f"{name}_weights"])


def trim_count(boxes):
    """boxes (M, C) without the class column -> number of kept rows (the last row >= 1 whose fp32 left-to-right sum is not 0)"""
    cnt = boxes.shape[0] - 1
    while cnt > 0:
        s = f32(0)
        for v in boxes[cnt]:
            s = f32(s + f32(v))
        if s != 0:
            break
        cnt -= 1
    return cnt + 1


def distances(anchors, gts):
    d = anchors[:, None, 0:3].astype(f32) - gts[None, :, 0:3].astype(f32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def topk_candidates(dist_col, topk):
    """indices of the topk smallest (distance, index)"""
    return np.lexsort((np.arange(dist_col.shape[0]), dist_col))[:topk]


def threshold(cand_iou):
    topk = cand_iou.shape[0]
    s = f32(0)
    for v in cand_iou:
        s = f32(s + v)
    mean = f32(s / f32(topk))
    ss = f32(0)
    for v in cand_iou:
        dv = f32(v - mean)
        ss = f32(ss + f32(dv * dv))
    return f32(f32(mean + f32(np.sqrt(f32(ss / f32(topk - 1))))) + f32(1e-6))


def centre_inside(anchors, g):
    """anchor centres inside gt `g` in BEV as the reference tests it: the offset rotated by -heading, x against dy / 2 and y
    against dx / 2 (the reference's column swap, atss_target_assigner.py:109), both inclusive"""
    c, s = f32(np.cos(np.float64(g[6]))), f32(np.sin(np.float64(g[6])))
    lx, ly = (anchors[:, 0] - g[0]).astype(f32), (anchors[:, 1] - g[1]).astype(f32)
    rx = (lx * c + ly * s).astype(f32)
    ry = (lx * f32(-s) + ly * c).astype(f32)
    hx, hy = f32(g[3] / f32(2)), f32(g[4] / f32(2))
    return (rx <= hy) & (rx >= -hy) & (ry <= hx) & (ry >= -hx)


def encode(g, a, code_size, sincos):
    """ResidualCoder.encode_torch of gt rows g (n, >= 7) against anchors a (n, >= 7), fp32; log / sin / cos rounded once from double"""
    g, a = g.astype(f32), a.astype(f32)
    da = np.maximum(a[:, 3:6], f32(1e-5))
    dg = np.maximum(g[:, 3:6], f32(1e-5))
    diag = np.sqrt(da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]).astype(f32)
    cols = [(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / da[:, 2]]
    cols += [np.log((dg[:, q] / da[:, q]).astype(np.float64)).astype(f32) for q in range(3)]
    if sincos:
        cols += [np.cos(g[:, 6].astype(np.float64)).astype(f32) - np.cos(a[:, 6].astype(np.float64)).astype(f32),
                 np.sin(g[:, 6].astype(np.float64)).astype(f32) - np.sin(a[:, 6].astype(np.float64)).astype(f32)]
    else:
        cols += [g[:, 6] - a[:, 6]]
    e = 7
    while len(cols) < code_size:
        cols.append(g[:, e] - a[:, e])
        e += 1
    return np.stack(cols, axis=1).astype(f32)


def assign_single(anchors, gts, classes, ious, topk, code_size, sincos):
    """anchors (N, D), gts (m, C) trimmed, classes (m), ious (N, m) -> labels (N) int32, targets (N, code) f32, weights (N) f32"""
    N, m = anchors.shape[0], gts.shape[0]
    dist = distances(anchors, gts)
    value = np.full(N, -np.inf, np.float64)
    owner = np.zeros(N, np.int64)
    matched = np.zeros(N, bool)
    for j in range(m):
        cand = topk_candidates(dist[:, j], topk)
        ci = ious[cand, j].astype(f32)
        pos = (ci >= threshold(ci)) & centre_inside(anchors[cand], gts[j])
        for a, v in zip(cand[pos], ci[pos]):
            if v > value[a]:              # strict: the lowest gt keeps a tie
                value[a], owner[a], matched[a] = v, j, True
    for j in range(m):                     # in gt order: the highest gt keeps a shared anchor
        a = int(np.argmax(ious[:, j]))     # first maximum: the lowest anchor index, 0 when every IoU is 0
        owner[a], matched[a] = j, True
    labels = np.where(matched, classes[owner].astype(np.int32), 0).astype(np.int32)
    targets = np.zeros((N, code_size), f32)
    weights = np.zeros(N, f32)
    fg = labels > 0
    if fg.any():
        targets[fg] = encode(gts[owner[fg]], anchors[fg], code_size, sincos)
        weights[fg] = 1.0
    return labels, targets, weights


def assign(anchor_sets, gt, topk, code_size, sincos, iou_fn):
    """anchor_sets: [(n_k, D)] in output order; gt (B, M, C + 1); iou_fn(frame, set, anchors (n, 7), gts (m, 7)) -> (n, m) f32.
    -> labels (B, N) int32, targets (B, N, code) f32, weights (B, N) f32, the sets one after the other"""
    out = ([], [], [])
    for b in range(gt.shape[0]):
        boxes = gt[b, :, :-1]
        cnt = trim_count(boxes)
        g, cls = boxes[:cnt], gt[b, :cnt, -1]
        parts = [assign_single(a, g, cls, np.asarray(iou_fn(b, k, a[:, :7], g[:, :7]), f32), topk, code_size, sincos)
                 for k, a in enumerate(anchor_sets)]
        for o, q in zip(out, range(3)):
            o.append(np.concatenate([p[q] for p in parts], axis=0))
    return tuple(np.stack(o, axis=0) for o in out)


def iou3d_from_bev_overlap(overlap, a, g):
    """boxes_iou3d_gpu's formula (iou3d_nms_utils.py:48-81) from a BEV overlap matrix, fp32"""
    a, g = a.astype(f32), g.astype(f32)
    a_lo, a_hi = a[:, 2] - a[:, 5] / f32(2), a[:, 2] + a[:, 5] / f32(2)
    g_lo, g_hi = g[:, 2] - g[:, 5] / f32(2), g[:, 2] + g[:, 5] / f32(2)
    oh = np.maximum(np.minimum(a_hi[:, None], g_hi[None, :]) - np.maximum(a_lo[:, None], g_lo[None, :]), f32(0))
    s3 = (overlap.astype(f32) * oh).astype(f32)
    va, vg = a[:, 3] * a[:, 4] * a[:, 5], g[:, 3] * g[:, 4] * g[:, 5]
    return (s3 / np.maximum(va[:, None] + vg[None, :] - s3, f32(1e-6))).astype(f32)


def bev_overlap_from_iou(iou, a, g):
    """inverts iou = s / max(sa + sb - s, 1e-8) for the overlap s (double, rounded once)"""
    sa = (a[:, 3].astype(np.float64) * a[:, 4])[:, None]
    sb = (g[:, 3].astype(np.float64) * g[:, 4])[None, :]
    i = iou.astype(np.float64)
    return (i * (sa + sb) / (1.0 + i)).astype(f32)
