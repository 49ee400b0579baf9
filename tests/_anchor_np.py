"""Plain restatements of the two first-stage training kernels, taking the arguments of their C ABI (include/lidar_hip.h), and the
inputs tests/test_gpu_anchor_kernel_support.py feeds them.  CPU only: numpy for the assignment, float64 torch autograd for the loss.

  assign_np   AxisAlignedTargetAssigner.assign_targets per frame and anchor class: the decision path (aligned BEV box, area,
              intersection, IoU, first-maximum argmax, gt max of 0 -> -1, forced / matched / unmatched, fg taken before the
              background pass) in np.float32 in the reference's expression order, a float64 shadow of every IoU matrix next to it,
              and the targets in float64 (plus the fp32 expression of the columns that have to be bit-equal).
  loss_np     the three RPN loss terms and their gradients with respect to every cls / box / dir tensor, in float64.

Both are trusted only after they reproduce the committed fixtures (tests/test_anchor_kernel_args_host.py).

Test inputs sit on a dyadic lattice (anchor and gt centres and sizes are multiples of 1/8), so BEV boxes, areas and intersections
are exact in fp32 and only the IoU's division rounds.  `assign_precondition` states, from the float64 shadow, what a case has to
satisfy before anything is launched."""
import functools
import math
import os
import re

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidardetection_amd", "csrc")
ID_MIN, NUM_IDS = -64, 128


def frames_per_block():
    """the assignment launcher's split of the batch over blockIdx.y, read from the launcher itself"""
    with open(os.path.join(CSRC, "anchor_assign.hip")) as f:
        found = re.findall(r"\.frames_per_block\s*=\s*(\d+)\s*;", f.read())
    assert len(found) == 1, found
    return int(found[0])


# ------------------------------------------------------------------------------------------------ assignment
def _aligned_bev(boxes, dt):
    """(n, >= 7) boxes -> (n, 4) x1 y1 x2 y2 of the axis-aligned BEV box, and |heading folded to [-pi/2, pi/2)|"""
    b = boxes.astype(dt)
    pi = dt(np.pi)
    rot = np.abs(b[:, 6] - np.floor(b[:, 6] / pi + dt(0.5)) * pi)
    keep = rot < dt(np.pi / 4)
    ex, ey = np.where(keep, b[:, 3], b[:, 4]), np.where(keep, b[:, 4], b[:, 3])
    two = dt(2)
    return np.stack([b[:, 0] - ex / two, b[:, 1] - ey / two, b[:, 0] + ex / two, b[:, 1] + ey / two], axis=1), rot


def _iou_matrix(ab, gb, dt):
    w = np.maximum(np.minimum(ab[:, None, 2], gb[None, :, 2]) - np.maximum(ab[:, None, 0], gb[None, :, 0]), dt(0))
    h = np.maximum(np.minimum(ab[:, None, 3], gb[None, :, 3]) - np.maximum(ab[:, None, 1], gb[None, :, 1]), dt(0))
    inter = w * h
    area_a = (ab[:, 2] - ab[:, 0]) * (ab[:, 3] - ab[:, 1])
    area_g = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
    return inter / np.maximum(area_a[:, None] + area_g[None, :] - inter, dt(F32(1e-6)))


def _encode(g, a, code_size, sincos, dt):
    """the residual box code of gt rows g against anchor rows a (same length)"""
    g, a = g.astype(dt), a.astype(dt)
    floor = dt(F32(1e-5))
    da, dg = np.maximum(a[:, 3:6], floor), np.maximum(g[:, 3:6], floor)
    diag = np.sqrt(da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1])
    out = np.zeros((len(a), code_size), dt)
    out[:, 0] = (g[:, 0] - a[:, 0]) / diag
    out[:, 1] = (g[:, 1] - a[:, 1]) / diag
    out[:, 2] = (g[:, 2] - a[:, 2]) / da[:, 2]
    out[:, 3:6] = np.log(dg / da)
    if sincos:
        out[:, 6] = np.cos(g[:, 6]) - np.cos(a[:, 6])
        out[:, 7] = np.sin(g[:, 6]) - np.sin(a[:, 6])
        q = 8
    else:
        out[:, 6] = g[:, 6] - a[:, 6]
        q = 7
    extra = code_size - q
    if extra:
        out[:, q:] = g[:, 7:7 + extra] - a[:, 7:7 + extra]
    return out


def approx_columns(sincos):
    """target columns that go through log / sin / cos (compared within 1e-6 of float64); the others are bit-equal to fp32"""
    return [3, 4, 5] + ([6, 7] if sincos else [])


def _row_sum32(row):
    s = F32(0)
    for v in row:
        s = F32(s + F32(v))
    return s


def assign_np(anchors, counts, per_loc, out_off, matched, unmatched, remap, num_classes, anchor_dim, a_total, class_of_id, gt,
              gt_enlarged, batch, max_gt, gt_cols, code_size, sincos, norm_by_num_examples):
    """The arguments of lidar_anchor_assign, with numpy arrays for the device pointers (anchors: a list of (counts[k], anchor_dim)
    float32 arrays; gt / gt_enlarged (batch, max_gt, gt_cols) float32, gt None when max_gt == 0).
    -> dict: labels (B, N) int32, weights (B, N) float32, targets (B, N, code) float64, targets32 (B, N, code) float32 (the fp32
    expression), shadow: one entry per (frame, class) that has gts: b, k, iou32, iou64, rot64 of its gts, their rows and labels."""
    K = num_classes
    assert code_size == 6 + (2 if sincos else 1) + min(anchor_dim, gt_cols - 1) - 7
    n_total = int(sum(counts))
    labels = np.full((batch, n_total), np.iinfo(np.int32).min, np.int32)
    weights = np.full((batch, n_total), np.nan, F32)
    targets = np.full((batch, n_total, code_size), np.nan, np.float64)
    targets32 = np.full((batch, n_total, code_size), np.nan, F32)
    table = [int(v) for v in class_of_id]
    assert len(table) == NUM_IDS
    bev32 = [_aligned_bev(a, F32)[0] for a in anchors]
    bev64 = [_aligned_bev(a, np.float64) for a in anchors]
    out_index = []
    for k in range(K):
        i = np.arange(int(counts[k]), dtype=np.int64)
        out_index.append((i // int(per_loc[k])) * int(a_total) + int(out_off[k]) + i % int(per_loc[k]))
    shadow = []
    for b in range(batch):
        n = max_gt
        while n > 1 and _row_sum32(gt[b, n - 1, :gt_cols - 1]) == 0:     # trailing padding rows; row 0 always stays
            n -= 1
        rows_of = [[] for _ in range(K)]
        label_of = [[] for _ in range(K)]
        for r in range(n):
            v = gt[b, r, gt_cols - 1]
            if not (v > F32(ID_MIN - 1) and v < F32(NUM_IDS + ID_MIN)):    # outside the id table (NaN included): no class
                continue
            cid = int(v)                                                   # truncates toward zero, as .int()
            k = table[cid - ID_MIN]
            if k < 0:
                continue
            rows_of[k].append(r)
            label_of[k].append(int(remap[k]) if remap[k] > 0 else cid)
        src = gt_enlarged if gt_enlarged is not None else gt
        for k in range(K):
            na = int(counts[k])
            if na == 0:
                continue
            a = anchors[k]
            lab = np.full(na, -1, np.int32)
            tg64 = np.zeros((na, code_size), np.float64)
            tg32 = np.zeros((na, code_size), F32)
            if rows_of[k]:
                rows = np.array(rows_of[k])
                gid = np.array(label_of[k], np.int32)
                g = gt[b, rows]
                gb32, _ = _aligned_bev(g, F32)
                gb64, grot64 = _aligned_bev(g, np.float64)
                iou = _iou_matrix(bev32[k], gb32, F32)
                assert iou.dtype == F32
                iou64 = _iou_matrix(bev64[k][0], gb64, np.float64)
                shadow.append(dict(b=b, k=k, iou32=iou, iou64=iou64, rot64=grot64, matched=F32(matched[k]),
                                   unmatched=F32(unmatched[k]), rows=rows, gid=gid))
                arg = iou.argmax(axis=1)                                   # the first maximum
                amax = iou[np.arange(na), arg]
                gmax = iou.max(axis=0).copy()
                gmax[gmax == 0] = -1                                       # a gt that overlaps no anchor forces nothing
                forced = (iou == gmax[None, :]).any(axis=1)
                pos = amax >= F32(matched[k])
                lab[forced] = gid[arg][forced]
                lab[pos] = gid[arg][pos]
                fg = lab > 0                                               # whose targets are encoded: before the background pass
                lab[amax < F32(unmatched[k])] = 0
                lab[forced] = gid[arg][forced]
                enc = src[b, rows][arg[fg]]
                tg64[fg] = _encode(enc, a[fg], code_size, sincos, np.float64)
                tg32[fg] = _encode(enc, a[fg], code_size, sincos, F32)
            else:
                lab[:] = 0
            w = np.zeros(na, F32)
            if norm_by_num_examples:
                w[lab > 0] = F32(1.0) / F32(max(int((lab >= 0).sum()), 1))
            else:
                w[lab > 0] = F32(1.0)
            o = out_index[k]
            labels[b, o], weights[b, o], targets[b, o], targets32[b, o] = lab, w, tg64, tg32
    return dict(labels=labels, weights=weights, targets=targets, targets32=targets32, shadow=shadow, out_index=out_index,
                anchor_rot64=[r for _, r in bev64])


IOU_MARGIN = 2e-6        # the margin the NMS tests use for a threshold decision
HEADING_MARGIN = 1e-4


def assign_precondition(ref):
    """What a case must satisfy so that an fp32 evaluation can be held to bit-equal labels: no IoU within IOU_MARGIN of a threshold
    (an IoU that IS the threshold, exactly and in both precisions, is a case built to sit on it and is decided the same way by
    both), no heading within HEADING_MARGIN of the dx / dy swap, and the fp32 IoU is the float64 one to rounding.  -> the share of
    anchors left out of the comparison, which is 0: nothing is masked."""
    for s in ref["shadow"]:
        assert np.abs(s["iou32"].astype(np.float64) - s["iou64"]).max(initial=0) <= 2.0 ** -23, (s["b"], s["k"])
        for thr in (s["matched"], s["unmatched"]):
            t64 = float(thr)
            near = np.abs(s["iou64"] - t64) <= IOU_MARGIN
            exact = (s["iou64"] == t64) & (s["iou32"] == thr)
            assert not (near & ~exact).any(), (s["b"], s["k"], t64, s["iou64"][near & ~exact][:4])
        assert (np.abs(s["rot64"] - np.pi / 4) > HEADING_MARGIN).all(), (s["b"], s["k"])
    for rot in ref["anchor_rot64"]:
        assert (np.abs(rot - np.pi / 4) > HEADING_MARGIN).all()
    return 0.0


def class_table(num_names, name_of_class):
    """the (128) id table of a name list of num_names entries, where anchor class k carries name index name_of_class[k]: gt id c
    reads names[c - 1] with numpy's wrap; ids past the list (or outside -64..63) match nothing"""
    cls_of_name = {n: k for k, n in enumerate(name_of_class)}
    assert len(cls_of_name) == len(name_of_class)
    table = []
    for cid in range(ID_MIN, ID_MIN + NUM_IDS):
        j = cid - 1
        table.append(cls_of_name.get(j % num_names, -1) if -num_names <= j < num_names else -1)
    return table


# the assignment cases: every axis value of the issue appears in at least one (test_assign_cases_cover_every_axis_value).
# layout: ("single", locs, per_loc) -> counts = locs * per_loc, interleaved out_off; ("multi", counts) -> per_loc = counts, running
# offsets; ("multi_rev", counts) -> the class blocks in reverse order.  dims: (anchor_dim, gt_cols, sincos).  batch: a number, or
# ("F", d) -> frames_per_block + d, ("2F", d) -> 2 * frames_per_block + d.  thr0: (matched, unmatched) of class 0, which holds the
# hand-placed anchors (IoU exactly 1 and exactly 0.5 against the hand-placed gt).
ASSIGN_CASES = {
    "c1_single_nogt": dict(layout=("single", 257, (1,)), dims=(7, 8, 0), max_gt=0, batch=1, thr0=(0.6013, 0.4507)),
    "c1_multi_m1": dict(layout=("multi", (513,)), dims=(7, 8, 1), max_gt=1, batch=("F", 0), thr0=(0.6013, 0.4507), norm=1),
    "c2_single_m63": dict(layout=("single", 255, (2, 4)), dims=(9, 10, 0), max_gt=63, batch=("F", -1), thr0=(0.5, 0.3491)),
    "c2_multi_m64_code11": dict(layout=("multi", (256, 1)), dims=(11, 12, 0), max_gt=64, batch=("F", 1), thr0=(0.6013, 0.5), enlarged=1),
    "c3_single_m65": dict(layout=("single", 256, (1, 2, 4)), dims=(9, 10, 1), max_gt=65, batch=1, thr0=(0.5, 0.5), norm=1,
                          remap=(2, 0, 1)),
    "c3_multi_m255_code13": dict(layout=("multi", (255, 256, 257)), dims=(12, 13, 1), max_gt=255, batch=("2F", 1), thr0=(0.3007, 0.6013),
                                 remap=(1, 1, 2)),
    "c10_multi_m256_ids": dict(layout=("multi", (255, 1, 256, 257, 0, 513, 1, 0, 256, 2)), dims=(16, 17, 0), max_gt=256, batch=1,
                               thr0=(0.6013, 0.4507), names=65, name_of_class=(5, 63, 62, 0, 60, 59, 58, 57, 56, 64), enlarged=1),
    "c10_rev_m257_neg": dict(layout=("multi_rev", (256, 1, 255, 513, 0, 257, 1, 2, 0, 256)), dims=(15, 16, 1), max_gt=257,
                             batch=("F", 0), thr0=(0.5, 0.5), norm=1, neg_frame=(1, 1)),
    "c16_multi_m600_code15": dict(layout=("multi", (256, 513, 1, 0, 255, 257, 3, 0, 1, 256, 2, 5, 257, 0, 64, 255)),
                                  dims=(15, 16, 0), max_gt=600, batch=("F", -1), thr0=(0.6013, 0.4507), enlarged=1,
                                  heavy={0: (1, 513), 1: (1, 257), 2: (1, 513)}, norm=1),
    "c16_single_m64": dict(layout=("single", 1, (1, 2, 4, 1, 2, 4, 1, 2, 4, 1, 2, 4, 1, 2, 4, 1)), dims=(9, 8, 0), max_gt=64,
                           batch=("F", 1), thr0=(0.6013, 0.4507)),
    "c3_single_m65_zero": dict(layout=("single", 513, (1, 1, 2)), dims=(7, 10, 0), max_gt=65, batch=("F", -1),
                               thr0=(0.6013, 0.4507), zero_frame=1),
    "c2_multi_m63_zero": dict(layout=("multi", (257, 255)), dims=(7, 8, 0), max_gt=63, batch=("F", 1), thr0=(0.6013, 0.4507),
                              zero_frame=1, enlarged=1, remap=(0, 3)),
    # odd code sizes on interleaved layouts with full 256-anchor tiles: there the target store's anchor-of-element quotient picks
    # the output row (on a multihead layout the row is off + quotient, and the quotient cancels out of the address)
    "c2_single_m64_code13": dict(layout=("single", 256, (2, 4)), dims=(12, 13, 1), max_gt=64, batch=1, thr0=(0.6013, 0.4507)),
    "c3_single_m63_code11": dict(layout=("single", 256, (1, 2, 4)), dims=(11, 12, 0), max_gt=63, batch=1, thr0=(0.5, 0.3491),
                                 enlarged=1),
    "c2_single_m65_code15": dict(layout=("single", 128, (4, 2)), dims=(15, 16, 0), max_gt=65, batch=1, thr0=(0.6013, 0.4507)),
}
# seeds for which assign_precondition holds: the first of base, base + 1000, ... that passes, base = ASSIGN_SEED_BASE + the case's
# position (no case was changed for it; first_good_seed finds them, and a host test holds the list to it)
ASSIGN_SEED_BASE = 700
ASSIGN_SEEDS = dict(zip(ASSIGN_CASES, (700, 701, 702, 703, 704, 1705, 706, 707, 708, 709, 710, 711, 712, 713, 714)))
# off the small rationals the lattice's IoUs fall on (3/5, 9/20, ...), so that a seed exists; 0.5 is exact and stays
OTHER_THRESHOLDS = [(0.6013, 0.4507), (0.5, 0.3491), (0.5513, 0.4009)]
SPECIAL_IDS = (-1.0, -64.0, 63.0, 64.0, -65.0, 1e9, 1.9, -0.5)     # + one id past the name list
TIE_X = 1000.0           # where the hand-placed anchors and their gt live, far from the lattice
FAR_XY = 3000.0          # a gt that overlaps no anchor


def resolve_batch(b):
    if isinstance(b, tuple):
        return {"F": 1, "2F": 2}[b[0]] * frames_per_block() + b[1]
    return b


def case_layout(spec):
    kind = spec["layout"][0]
    if kind == "single":
        _, locs, per = spec["layout"]
        counts = [locs * r for r in per]
        off = [int(x) for x in np.cumsum([0] + list(per[:-1]))]
        return counts, list(per), off, sum(per)
    counts = list(spec["layout"][1])
    total = max(sum(counts), 1)
    if kind == "multi":
        off = [int(x) for x in np.cumsum([0] + counts[:-1])]
    else:
        off = [int(x) for x in (np.cumsum([0] + counts[::-1][:-1]))][::-1]
    return counts, [max(n, 1) for n in counts], off, total


def build_assign_case(name, seed):
    """-> the keyword arguments of assign_np for the case"""
    spec = ASSIGN_CASES[name]
    r = np.random.default_rng(seed)
    counts, per_loc, out_off, a_total = case_layout(spec)
    K = len(counts)
    D, gt_cols, sincos = spec["dims"]
    code = 6 + (2 if sincos else 1) + min(D, gt_cols - 1) - 7
    B, M = resolve_batch(spec["batch"]), spec["max_gt"]
    L = spec.get("names", K + 1)                       # one spare name without an anchor class: its gts match nothing
    name_of_class = list(spec.get("name_of_class", [L - 1 - k for k in range(K)]))
    table = class_table(L, name_of_class)
    # the id of class k: its name's own, or, past the id table, the negative id that wraps to the same name (so does id_of[k] - L)
    id_of = [n + 1 if n + 1 < NUM_IDS + ID_MIN else n + 1 - L for n in name_of_class]
    anchors = []
    for k, n in enumerate(counts):
        i = np.arange(n)
        a = np.zeros((n, D), F32)
        a[:, 0], a[:, 1] = (i % 32) * 0.5, (i // 32) * 0.5
        a[:, 2] = -1 + 0.125 * (k % 8)
        a[:, 3], a[:, 4], a[:, 5] = 1 + 0.25 * (k % 5), 0.5 + 0.125 * (k % 3), 1.5 + 0.125 * (k % 2)
        a[:, 6] = np.where(i % 2 == 0, 0.0, 1.57)
        a[:, 7:] = r.integers(-8, 9, (n, D - 7)) / 8
        anchors.append(a)
    tie = counts[0] >= 3
    if tie:     # anchor 0: the tie gt's own box (IoU 1, forced); anchor 1: half of it (IoU exactly 0.5, not forced)
        anchors[0][0, :7] = [TIE_X, 0, -1, 2, 2, 1.5, 0]
        anchors[0][1, :7] = [TIE_X, 0, -1, 2, 1, 1.5, 0]
    live = [k for k in range(K) if counts[k] > 0]

    def jittered(k):
        a = anchors[k][int(r.integers(2 if (tie and k == 0) else 0, counts[k]))]
        g = np.zeros(gt_cols, F32)
        g[:7] = a[:7]
        g[:3] += r.integers(-4, 5, 3) / 8
        g[3:6] += r.integers(-2, 3, 3) / 8
        g[6] = r.uniform(-np.pi, np.pi)
        g[7:gt_cols - 1] = r.integers(-16, 17, gt_cols - 8) / 8
        g[-1] = id_of[k]
        return g

    gt = np.zeros((B, M, gt_cols), F32) if M else None
    for b in range(B if M else 0):
        if spec.get("zero_frame") and b == B - 1:
            continue                                                       # an all-zero frame
        heavy = spec.get("heavy", {}).get(b)
        n = M if b == 0 or heavy else int(r.integers(0, M + 1))            # frame 0 is full, the others end in zero rows
        if M == 1:
            n = 1 - b % 2                                                  # max_gt == 1: a real row, then a zero row
        cls = r.choice(live, n)
        if heavy:                                                          # exactly hn gts of class hk past the special rows
            hk, hn = heavy
            cls = r.choice([k for k in live if k != hk], n)
            cls[24 + r.choice(n - 24, hn, replace=False)] = hk
        for j in range(n):
            gt[b, j] = jittered(int(cls[j]))
        if heavy and heavy[1] > 300:     # two identical gts more than 256 slots apart in their class: the first must win.  Both
            rows = np.nonzero(cls == heavy[0])[0]       # are an anchor's own box (IoU 1: they decide that anchor), and the copy
            gt[b, rows[40], :7] = anchors[heavy[0]][counts[heavy[0]] // 4 + b, :7]   # carries the wrapped id, so the winner shows
            gt[b, rows[340]] = gt[b, rows[40]]                                       # in the label
            gt[b, rows[340], -1] -= L
        if b == 0 and M >= 63:
            kc = max(live, key=lambda k: counts[k])
            sp = []
            g = jittered(kc); g[:7] = anchors[kc][counts[kc] // 2, :7]; sp.append(g)                 # a gt copied from an anchor
            for sgn in (1, -1):                                                                       # two gts with the same IoU
                g = jittered(kc); g[:7] = anchors[kc][counts[kc] // 3, :7]; g[0] += sgn * 0.125; sp.append(g)
            g = jittered(kc); sp.append(g); g2 = g.copy(); g2[-1] -= L; sp.append(g2)                 # two identical gts
            sp.append(np.zeros(gt_cols, F32))                                                         # a zero row between real ones
            g = jittered(kc); g[0] = g[1] = FAR_XY; sp.append(g)                                      # overlaps no anchor
            for cid in SPECIAL_IDS + (float(L + 1),):
                g = jittered(kc); g[-1] = cid; sp.append(g)
            if tie:
                g = jittered(0); g[:7] = [TIE_X, 0, -1, 2, 2, 1.5, 0.1]; sp.append(g)
            gt[0, 2:2 + len(sp)] = np.stack(sp)
        if spec.get("neg_frame") and spec["neg_frame"][0] == b:            # every gt of one class carries the wrapped id: with
            k = spec["neg_frame"][1]                                       # remap 0 its anchors' labels are negative or ignored
            ids = gt[b, :, -1]
            ids[ids == id_of[k]] = id_of[k] - L
    enl = None
    if spec.get("enlarged") and M:
        enl = gt.copy()
        real = np.abs(gt[:, :, :gt_cols - 1]).sum(-1) > 0
        enl[:, :, 0:3] += np.where(real[..., None], r.integers(-2, 3, (B, M, 3)) / 8, 0).astype(F32)
        enl[:, :, 3:6] += np.where(real[..., None], r.integers(0, 4, (B, M, 3)) / 8, 0).astype(F32)
    thr = [spec["thr0"]] + [OTHER_THRESHOLDS[k % 3] for k in range(1, K)]
    return dict(anchors=anchors, counts=counts, per_loc=per_loc, out_off=out_off, matched=[t[0] for t in thr],
                unmatched=[t[1] for t in thr], remap=list(spec.get("remap", [0] * K)), num_classes=K, anchor_dim=D,
                a_total=a_total, class_of_id=table, gt=gt, gt_enlarged=enl, batch=B, max_gt=M, gt_cols=gt_cols, code_size=code,
                sincos=sincos, norm_by_num_examples=int(spec.get("norm", 0)))


@functools.lru_cache(maxsize=None)
def assign_case(name):
    """(arguments, reference) of a committed case; the reference is computed once and shared"""
    args = build_assign_case(name, ASSIGN_SEEDS[name])
    return args, assign_np(**args)


def first_good_seed(name, base, tries=20):
    for s in range(base, base + 1000 * tries, 1000):
        try:
            assign_precondition(assign_np(**build_assign_case(name, s)))
            return s
        except AssertionError:
            continue
    raise AssertionError(f"no seed for {name}")


# ------------------------------------------------------------------------------------------------ loss
def loss_np(cls, box, dirs, counts, cols, col_off, labels, targets, anchors, num_class, code_size, num_dir_bins, code_weights,
            weights, flags, grad_losses=(1.0, 1.0, 1.0)):
    """The arguments of lidar_anchor_loss_forward / _backward with numpy arrays for the device pointers (cls / box / dirs: lists of
    per-head (B, counts[k], .) arrays, dirs None without bit 4).  The host scalars are used as given (callers that compare with the
    kernels pass fp32-representable values); code_weights pass through fp32, as the reference's buffer does.  The math is float64.
    -> losses (3) float64, grads: dict cls / box / dir -> per-head float64 arrays of d(sum_i grad_losses[i] * losses[i])."""
    import torch
    f64 = lambda v: torch.from_numpy(np.asarray(v, F32).astype(np.float64))   # noqa: E731
    H = len(counts)
    B, N = labels.shape
    w_cls, w_loc, w_dir, pos_w, neg_w, dir_off, dir_bin = [float(v) for v in weights]
    sin_diff, l1, use_dir = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    lab = torch.from_numpy(labels.astype(np.int64))
    if num_class == 1:
        lab = torch.where(lab > 0, torch.ones_like(lab), lab)             # a class-agnostic head: every positive is class 1
    pos, neg = (lab > 0).double(), (lab == 0).double()
    norm = pos.sum(1, keepdim=True).clamp(min=1.0)                        # per frame, at least 1
    norm32 = norm.numpy().astype(F32)       # the reference's class and box weights are fp32 tensors whatever the predictions are
    cw = f64(code_weights)[:code_size]
    tg_all = f64(targets)
    xs = [f64(x).requires_grad_() for x in cls]
    bs = [f64(x).requires_grad_() for x in box]
    ds = [f64(x).requires_grad_() for x in dirs] if use_dir else []
    beta = 1.0 / 9.0
    lc = ll = ld = torch.zeros((), dtype=torch.float64)
    a0 = 0
    for h in range(H):
        n, c = int(counts[h]), int(cols[h])
        lb, ps = lab[:, a0:a0 + n], pos[:, a0:a0 + n]
        col = torch.arange(c)[None, None, :] + int(col_off[h]) + 1
        t = ((lb[..., None] >= 0) & (lb[..., None] == col)).double()      # one-hot of the head's own class columns
        x = xs[h]
        p = torch.sigmoid(x)
        alpha = t * 0.25 + (1 - t) * 0.75
        pt = t * (1 - p) + (1 - t) * p
        bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
        anchor_w = f64((ps * pos_w + neg[:, a0:a0 + n] * neg_w).numpy().astype(F32) / norm32)   # fp32 weights in the reference
        lc = lc + (alpha * pt * pt * bce * anchor_w[..., None]).sum()
        pb, tg = bs[h], tg_all[:, a0:a0 + n]
        if sin_diff:      # sin(a - b) = sin a cos b - cos a sin b, split between prediction and target
            t32 = torch.from_numpy(np.ascontiguousarray(targets[:, a0:a0 + n, 6:7], F32))   # the target's side stays fp32 there
            s = torch.sin(pb[..., 6:7]) * torch.cos(t32).double()
            cc = torch.cos(pb[..., 6:7]) * torch.sin(t32).double()
            pb = torch.cat([pb[..., :6], s, pb[..., 7:]], dim=-1)
            tgb = torch.cat([tg[..., :6], cc, tg[..., 7:]], dim=-1)
        else:
            tgb = tg
        tgb = torch.where(torch.isnan(tgb), pb, tgb)                      # a NaN target takes the prediction: the term is 0
        d = ((pb - tgb) * cw).abs()
        if not l1:
            d = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
        ll = ll + (d * f64(ps.numpy().astype(F32) / norm32)[..., None]).sum()
        if use_dir:
            # the direction class is a decision: fp32, in the reference's expression order (dir_bin_margin keeps the test inputs
            # away from the bin edges, where fp32 and exact arithmetic may part)
            v = (targets[:, a0:a0 + n, 6].astype(F32) + anchors[None, a0:a0 + n, 6].astype(F32)) - F32(dir_off)
            rr = v - np.floor(v / F32(2 * math.pi)) * F32(2 * math.pi)
            k = torch.from_numpy(np.floor(rr / F32(dir_bin)).astype(np.int64)).clamp(0, num_dir_bins - 1)
            ce = -torch.log_softmax(ds[h], dim=-1).gather(-1, k[..., None]).squeeze(-1)
            ld = ld + (ce * (ps / norm)).sum()
        a0 += n
    assert a0 == N
    losses = torch.stack([lc / B * w_cls, ll / B * w_loc, ld / B * w_dir])
    g = torch.tensor([float(v) for v in grad_losses], dtype=torch.float64)
    leaves = xs + bs + ds
    grads = torch.autograd.grad((losses * g).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
    out = dict(cls=[x.numpy() for x in grads[:H]], box=[x.numpy() for x in grads[H:2 * H]], dir=[x.numpy() for x in grads[2 * H:]])
    return losses.detach().numpy(), out


def dir_bin_margin(targets, anchors, labels, weights, num_dir_bins):
    """float64 distance of every positive anchor's direction value to the nearest bin edge, in radians (the loss cases keep it
    above 1e-4, so fp32 and float64 pick the same bin)"""
    dir_off, dir_bin = float(weights[5]), float(weights[6])
    v = targets[..., 6].astype(np.float64) + anchors[None, :, 6].astype(np.float64) - dir_off
    rr = v - np.floor(v / (2 * np.pi)) * (2 * np.pi)
    q = rr / abs(dir_bin)
    edge = np.minimum(q - np.floor(q), np.ceil(q) - q) * abs(dir_bin)
    edge = np.minimum(edge, np.minimum(rr, 2 * np.pi - rr))
    return edge[labels > 0].min(initial=np.inf)


# counts / cols / col_off per head, num_class, code_size, bins, flags, batch and what the case adds.  Every axis value of the issue
# appears (test_loss_cases_cover_every_axis_value).  dir_bin_scale: weights[6] = scale * 2 pi / bins (0.5: the upper half of the
# circle needs the clamp at bins - 1; -1: every value needs the clamp at 0).
LOSS_CASES = {
    "f0_h1_agnostic": dict(counts=(257,), cols=(1,), col_off=(0,), num_class=1, code=7, bins=0, flags=0, batch=1),
    "f1_h2_sep": dict(counts=(255, 1000), cols=(1, 2), col_off=(0, 1), num_class=3, code=8, bins=0, flags=1, batch=2,
                      null_dbox=1, pos_neg=(1.0, 2.0)),
    "f2_h10_l1": dict(counts=(1, 255, 256, 257, 1000, 1, 2, 255, 3, 256), cols=(10,) * 10, col_off=(0,) * 10, num_class=10, code=9,
                      bins=0, flags=2, batch=5, frames=("nopos", "ignored", "allpos"), grad=(1.5, 0.0, 0.5)),
    "f3_h16_sep": dict(counts=(1, 2, 255, 3, 256, 1, 257, 5, 1, 64, 1, 7, 1000, 1, 2, 1), cols=(1,) * 16, col_off=tuple(range(16)),
                       num_class=16, code=10, bins=0, flags=3, batch=2, null_dcls_entry=3, pos_neg=(2.0, 0.5)),
    "f4_h1_bins1": dict(counts=(1000,), cols=(16,), col_off=(0,), num_class=16, code=16, bins=1, flags=4, batch=1, dir_off=0.0),
    "f5_h2_bins2": dict(counts=(256, 257), cols=(10, 3), col_off=(0, 10), num_class=13, code=7, bins=2, flags=5, batch=5,
                        frames=("allpos", "nopos", "ignored"), dir_off=0.78539, grad=(0.7, -1.3, 2.0)),
    "f6_h10_bins3_clamp_hi": dict(counts=(255, 1, 256, 2, 257, 1, 1, 3, 1, 1000), cols=(2, 1, 1, 2, 1, 1, 2, 1, 2, 3),
                                  col_off=(0, 2, 3, 4, 6, 7, 8, 10, 11, 13), num_class=16, code=9, bins=3, flags=6, batch=2,
                                  dir_off=0.78539, dir_bin_scale=0.5, pos_neg=(1.0, 2.0)),
    "f7_h16_bins8": dict(counts=(64, 1, 255, 1, 256, 2, 257, 1, 3, 1, 5, 1, 1000, 1, 2, 1), cols=(16,) * 16, col_off=(0,) * 16,
                         num_class=16, code=16, bins=8, flags=7, batch=1, dir_off=0.3),
    "f5_h2_bins2_clamp_lo": dict(counts=(257, 255), cols=(3, 3), col_off=(0, 0), num_class=3, code=8, bins=2, flags=5, batch=2,
                                 dir_off=0.78539, dir_bin_scale=-1.0),
}
LOSS_SEED = 900


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> (arguments of loss_np as a dict, (losses, grads) of loss_np); computed once and shared"""
    spec = LOSS_CASES[name]
    r = np.random.default_rng(LOSS_SEED + list(LOSS_CASES).index(name))
    counts, cols, B, code, bins, nc = spec["counts"], spec["cols"], spec["batch"], spec["code"], spec["bins"], spec["num_class"]
    N = sum(counts)
    labels = r.choice(np.arange(-1, nc + 1), (B, N), p=[0.1, 0.7] + [0.2 / nc] * nc).astype(np.int32)
    if nc == 1:
        labels[labels > 0] = r.integers(1, 4, int((labels > 0).sum()))      # a class-agnostic head sees the gts' own ids
    for b, kind in enumerate(spec.get("frames", ())):
        if kind == "nopos":
            labels[b] = np.minimum(labels[b], 0)
        elif kind == "ignored":
            labels[b] = -1
        else:
            labels[b] = r.integers(1, nc + 1, N)
    code_w = r.choice([1.0, 0.5, 2.0, 0.2], code).astype(F32)
    code_w[0] = code_w[1] = 1.0
    code_w[code - 1] = 0.0                                                   # a column that does not count
    targets = (r.integers(-16, 17, (B, N, code)) / 8).astype(F32)
    resid = (r.normal(0, 0.5, (B, N, code))).astype(F32)
    anchors = np.zeros((N, 9), F32)
    anchors[:, :6] = r.uniform(0.5, 4, (N, 6))
    anchors[:, 6] = np.where(np.arange(N) % 2 == 0, 0.0, 1.57)
    special = r.integers(0, 8, (B, N))       # columns 0 / 1 (code weight 1, never the heading) carry the exact residuals
    joint = F32(1.0 / 9.0)
    for kind, val in ((0, F32(0)), (1, joint), (2, -joint), (3, F32(10))):
        m = special == kind
        targets[m, 0] = 0
        resid[m, 0] = val
        targets[m, 1] = 0
        resid[m, 1] = -val
    nan_at = r.integers(0, 16, (B, N)) == 0
    targets[nan_at, 2] = np.nan                                              # a missing target (never the heading column)
    weights = [1.0, 2.0, float(F32(0.2)), *spec.get("pos_neg", (1.0, 1.0)), float(F32(spec.get("dir_off", 0.0))), 0.0]
    if bins:                                 # every host scalar is an fp32 number, so the kernel sees the reference's values
        width = 2 * np.pi / bins
        weights[6] = float(F32(spec.get("dir_bin_scale", 1.0) * width))
        k = r.integers(0, bins, (B, N))
        frac = r.uniform(0.05, 0.95, (B, N))
        if 0 < spec.get("dir_bin_scale", 1.0) < 1:      # narrower bins: stay inside them too
            k = k * 2 + r.integers(0, 2, (B, N))
            width = abs(weights[6])
        turn = r.integers(-1, 2, (B, N)) * 2 * np.pi
        targets[..., 6] = ((k + frac) * width + weights[5] - anchors[None, :, 6] + turn).astype(F32)
    box_t = np.where(np.isnan(targets), F32(0), targets) + resid
    cls, box, dirs = [], [], []
    a0 = 0
    for n, c in zip(counts, cols):
        x = (r.normal(0, 2, (B, n, c)) - 2).astype(F32)
        big = r.integers(0, 12, x.shape)
        x[big == 0], x[big == 1] = 50.0, -50.0
        cls.append(x)
        box.append(np.ascontiguousarray(box_t[:, a0:a0 + n]).astype(F32))
        if bins:
            dirs.append(r.normal(0, 1.5, (B, n, bins)).astype(F32))
        a0 += n
    args = dict(cls=cls, box=box, dirs=dirs if bins else None, counts=list(counts), cols=list(cols), col_off=list(spec["col_off"]),
                labels=labels, targets=targets, anchors=anchors, num_class=nc, code_size=code, num_dir_bins=bins,
                code_weights=code_w, weights=weights, flags=spec["flags"], grad_losses=spec.get("grad", (1.0, 1.0, 1.0)))
    return args, loss_np(**args)


# ------------------------------------------------------------------------------------------------ coverage of the axes
def assert_assign_cases_cover():
    F = frames_per_block()
    built = {name: assign_case(name)[0] for name in ASSIGN_CASES}
    specs = ASSIGN_CASES.values()
    refs = {name: assign_case(name)[1] for name in ASSIGN_CASES}
    assert {a["num_classes"] for a in built.values()} >= {1, 2, 3, 10, 16}
    assert {n for a in built.values() for n in a["counts"]} >= {0, 1, 255, 256, 257, 513}
    single = [s for s in specs if s["layout"][0] == "single"]
    assert {r for s in single for r in s["layout"][2]} >= {1, 2, 4} and any(s["layout"][0] == "multi" for s in specs)
    dims = {(*s["dims"], a["code_size"]) for s, a in zip(specs, built.values())}
    dims = {(*s["dims"], a["code_size"]) for s, a, ref in zip(specs, built.values(), refs.values())      # the cases that encode
            if (ref["labels"] > 0).any() and (np.abs(ref["targets"]).sum(-1) > 0).any()}                  # something
    assert dims >= {(7, 8, 0, 7), (7, 8, 1, 8), (9, 10, 0, 9), (9, 10, 1, 10), (16, 17, 0, 16), (15, 16, 1, 16), (9, 8, 0, 7),
                    (7, 10, 0, 7)}, dims
    for odd in (11, 13, 15):
        assert any(a["code_size"] == odd and 256 in a["counts"] for a in built.values()), odd        # on a 256-anchor tile
        seen = False        # and on an interleaved layout, full tiles, with targets in the upper half of a tile
        for s, a, ref in zip(specs, built.values(), refs.values()):
            if a["code_size"] != odd or s["layout"][0] != "single":
                continue
            for k, n in enumerate(a["counts"]):
                if a["per_loc"][k] > 1 and n % 256 == 0:
                    enc = (np.abs(ref["targets"][:, ref["out_index"][k]]).sum(-1) > 0).any(0)
                    seen |= bool(enc[np.arange(n) % 256 >= 128].any())
        assert seen, odd
    assert {a["max_gt"] for a in built.values()} >= {0, 1, 63, 64, 65, 255, 256, 257, 600}
    assert {a["batch"] for a in built.values()} >= {1, F - 1, F, F + 1, 2 * F + 1}
    assert any(a["gt_enlarged"] is not None for a in built.values()) and any(a["gt_enlarged"] is None for a in built.values())
    assert {a["norm_by_num_examples"] for a in built.values()} == {0, 1}
    assert any(max(a["remap"]) > 0 for a in built.values())
    thr0 = {(a["matched"][0], a["unmatched"][0]) for a in built.values()}
    assert any(m == 0.5 and u < m for m, u in thr0) and any(u == 0.5 and m > u for m, u in thr0)
    assert any(m < u for m, u in thr0) and any(m == u for m, u in thr0)
    per_class = []                          # gts of one class in one frame
    for a in built.values():
        if a["gt"] is None:
            continue
        for b in range(a["batch"]):
            ids = a["gt"][b, :, -1]
            real = np.abs(a["gt"][b, :, :-1]).sum(-1) > 0
            per_class += [int(((ids == v) & real).sum()) for v in np.unique(ids[real])]
    assert 257 in per_class and any(n >= 513 for n in per_class)


def assert_loss_cases_cover():
    specs = list(LOSS_CASES.values())
    assert {len(s["counts"]) for s in specs} >= {1, 2, 10, 16}
    assert {n for s in specs for n in s["counts"]} >= {1, 255, 256, 257, 1000}
    assert {c for s in specs for c in s["cols"]} >= {1, 2, 3, 10, 16}
    assert any(max(s["col_off"]) > 0 for s in specs)
    assert any(set(s["cols"]) == {s["num_class"]} and not any(s["col_off"]) for s in specs)
    assert {s["code"] for s in specs} >= {7, 8, 9, 10, 16}
    assert {s["bins"] for s in specs if s["flags"] & 4} >= {1, 2, 3, 8} and all(s["bins"] == 0 for s in specs if not s["flags"] & 4)
    assert {s["flags"] for s in specs} == set(range(8))
    assert {s["batch"] for s in specs} >= {1, 2, 5}
    assert {f for s in specs for f in s.get("frames", ())} == {"nopos", "ignored", "allpos"}
    assert any(s.get("dir_bin_scale", 1) == 0.5 for s in specs) and any(s.get("dir_bin_scale", 1) < 0 for s in specs)
    assert any(s.get("dir_off") for s in specs) and any(s.get("pos_neg", (1, 1))[0] != s.get("pos_neg", (1, 1))[1] for s in specs)
    assert any(0.0 in s.get("grad", ()) for s in specs) and any("null_dbox" in s for s in specs)
    assert any("null_dcls_entry" in s for s in specs)
