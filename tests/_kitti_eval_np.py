"""Numpy restatement of the KITTI AP evaluation around the overlaps (the reference's
pcdet/datasets/kitti/kitti_object_eval_python/eval.py: clean_data, compute_statistics_jit in both modes, get_thresholds, eval_class,
get_mAP / get_mAP_R40), written from the rules and not from its text, plus the loader of tests/golden/kitti_eval_ref.npz.  It takes
the overlaps as input (per frame a (dt, gt) float64 array); only the axis-aligned image overlap is restated here.

The matcher is written in the CLOSED FORM of each gt's choice, vectorised over the frame's dets, not as the reference's scan:
  pass 1 (thresh None)  among the dets that are of the class or too small (flag 0 or 1), unassigned and overlap > min_overlap:
                        the highest score, the lowest row on a tie
  pass 2 (thresh t)     the same set without the dets of score < t: among those with flag 0 the largest overlap, the lowest row on
                        a tie; if there is none, the first one with flag 1
tests/test_kitti_eval_host.py pins this to the reference's own curves, thresholds and counts."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kitti_eval_ref.npz")
CLASSES = ("car", "pedestrian", "cyclist", "van", "person_sitting", "truck")
DISPLAY = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck")
MIN_HEIGHT, MAX_OCCLUSION, MAX_TRUNCATION = (40, 25, 25), (0, 1, 2), (0.15, 0.3, 0.5)
PTS = 41
GT_KEYS = ("bbox", "location", "dimensions", "rotation_y", "alpha", "occluded", "truncated")
DT_KEYS = ("bbox", "location", "dimensions", "rotation_y", "alpha", "score")
OVERLAP_TABLE = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3,
                          [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]]])


def image_overlap(boxes, query, criterion=-1):
    """(N, 4) x (K, 4) axis-aligned boxes -> (N, K): intersection over union (-1), over the first box (0), the second (1)"""
    b, q = np.asarray(boxes, np.float64)[:, None, :], np.asarray(query, np.float64)[None, :, :]
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    barea, qarea = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]), (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    inter = iw * ih
    ua = {-1: barea + qarea - inter, 0: barea + 0 * qarea, 1: qarea + 0 * barea}[criterion]
    with np.errstate(all="ignore"):
        return np.where((iw > 0) & (ih > 0), inter / ua, 0.0)


def flags(gt, dt, cls, difficulty):
    """one frame -> (number of valid gts, gt flags, dt flags): 0 counts, 1 may be matched without counting, -1 takes no part"""
    want = CLASSES[cls]
    names = np.array([str(n).lower() for n in gt["name"]], dtype=object)
    own = names == want
    neighbour = names == {"car": "van", "pedestrian": "person_sitting"}.get(want, "\0")
    bbox = np.asarray(gt["bbox"], np.float64).reshape(-1, 4)
    hard = ((np.asarray(gt["occluded"], np.float64) > MAX_OCCLUSION[difficulty])
            | (np.asarray(gt["truncated"], np.float64) > MAX_TRUNCATION[difficulty])
            | (bbox[:, 3] - bbox[:, 1] <= MIN_HEIGHT[difficulty]))
    g = np.full(len(names), -1, np.int64)
    g[neighbour | (own & hard)] = 1
    g[own & ~hard] = 0
    dbox = np.asarray(dt["bbox"], np.float64).reshape(-1, 4)
    dnames = np.array([str(n).lower() for n in dt["name"]], dtype=object)
    d = np.where(np.abs(dbox[:, 3] - dbox[:, 1]) < MIN_HEIGHT[difficulty], 1, np.where(dnames == want, 0, -1)).astype(np.int64)
    return int((g == 0).sum()), g, d


def match(ov, gflag, dflag, scores, min_overlap, thresh=None, dc_ov=None, gt_alpha=None, dt_alpha=None):
    """one frame, one configuration.  thresh None -> list of (gt row, emitted score); else -> (tp, fp, fn, similarity sum)"""
    nd = len(dflag)
    live = dflag != -1
    if thresh is not None:
        live = live & (scores >= thresh)
    free = live.copy()
    emitted, tp, fn, sim = [], 0, 0, 0.0
    for i in np.nonzero(gflag != -1)[0]:
        cand = free & (ov[:, i] > min_overlap) if nd else free
        if thresh is None:
            cand = cand & (scores > -10000000)
            pick = int(np.argmax(np.where(cand, scores, -np.inf))) if cand.any() else -1
        else:
            first = cand & (dflag == 0)
            if first.any():
                pick = int(np.argmax(np.where(first, ov[:, i], -np.inf)))
            else:
                pick = int(np.argmax(cand)) if cand.any() else -1
        if pick < 0:
            fn += int(gflag[i] == 0)
            continue
        free[pick] = False
        if gflag[i] == 1 or dflag[pick] == 1:
            continue
        tp += 1
        emitted.append((int(i), float(scores[pick])))
        if gt_alpha is not None:
            sim += (1.0 + np.cos(gt_alpha[i] - dt_alpha[pick])) / 2.0
    if thresh is None:
        return emitted
    left = free & (dflag == 0)
    if dc_ov is not None and dc_ov.shape[1]:
        left = left & ~(dc_ov > min_overlap).any(1)
    return tp, int(left.sum()), fn, sim


def thresholds(scores, num_gt):
    """the score thresholds that sample the recall axis at 41 points: walk the scores downwards; score i gives recall (i + 1) /
    num_gt; it is taken when that recall is at least as close to the next sample point as the following score's recall is (the
    last score is always taken); each taken score moves the sample point on by 1 / 40 (by repeated addition)"""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    out, point = [], 0
    for i, v in enumerate(s):
        here = (i + 1) / num_gt
        last = i == len(s) - 1
        nxt = here if last else (i + 2) / num_gt
        if not last and (nxt - point) < (point - here):
            continue
        out.append(float(v))
        point += 1 / 40.0
    return out


def eval_class(gt_annos, dt_annos, classes, difficulties, metric, min_overlaps, overlaps, compute_aos=False):
    """min_overlaps (K, num_class) for this metric; overlaps: per frame (dt, gt).  -> dict: precision / recall / orientation
    (C, D, K, 41), thresholds [c][d][k] lists, counts (C, D, K, 41, 3) int64 tp / fp / fn, matched [c][d][k] lists of per-frame
    emitted (gt row, score) lists, num_valid_gt (C, D)"""
    C, D, K = len(classes), len(difficulties), len(min_overlaps)
    prec, rec, aos = (np.zeros((C, D, K, PTS)) for _ in range(3))
    counts = np.zeros((C, D, K, PTS, 3), np.int64)
    num_valid = np.zeros((C, D), np.int64)
    thr_all = [[[None] * K for _ in range(D)] for _ in range(C)]
    matched_all = [[[None] * K for _ in range(D)] for _ in range(C)]
    scores = [np.asarray(d["score"], np.float64) for d in dt_annos]
    dc = []
    for g, d in zip(gt_annos, dt_annos):
        rows = np.array([str(n) == "DontCare" for n in g["name"]], dtype=bool)
        dc.append(image_overlap(np.asarray(d["bbox"]).reshape(-1, 4), np.asarray(g["bbox"]).reshape(-1, 4)[rows], 0)
                  if metric == 0 else None)
    for m, cls in enumerate(classes):
        for l, diff in enumerate(difficulties):
            fl = [flags(g, d, cls, diff) for g, d in zip(gt_annos, dt_annos)]
            num_valid[m, l] = sum(f[0] for f in fl)
            for k in range(K):
                mo = float(min_overlaps[k][m])
                emitted = [match(overlaps[f], fl[f][1], fl[f][2], scores[f], mo) for f in range(len(gt_annos))]
                matched_all[m][l][k] = emitted
                thr = thresholds([s for e in emitted for _, s in e], num_valid[m, l])
                thr_all[m][l][k] = thr
                sims = np.zeros(len(thr))
                for f, (g, d) in enumerate(zip(gt_annos, dt_annos)):
                    for t, th in enumerate(thr):
                        tp, fp, fn, sim = match(overlaps[f], fl[f][1], fl[f][2], scores[f], mo, th, dc[f],
                                                np.asarray(g["alpha"], np.float64) if compute_aos else None,
                                                np.asarray(d["alpha"], np.float64))
                        counts[m, l, k, t] += (tp, fp, fn)
                        sims[t] += sim
                n = len(thr)
                tp, fp, fn = (counts[m, l, k, :n, q].astype(np.float64) for q in range(3))
                with np.errstate(all="ignore"):
                    curves = [tp / (tp + fp), tp / (tp + fn), sims / (tp + fp) if compute_aos else np.zeros(n)]
                for dst, cur in zip((prec, rec, aos), curves):
                    padded = np.concatenate([cur, np.zeros(PTS - n)])
                    for t in range(n):
                        dst[m, l, k, t] = np.max(padded[t:])
    return dict(precision=prec, recall=rec, orientation=aos, thresholds=thr_all, counts=counts, matched=matched_all,
                num_valid_gt=num_valid)


def map_r11(curve):
    return curve[..., ::4].sum(-1) / 11 * 100


def map_r40(curve):
    return curve[..., 1:].sum(-1) / 40 * 100


# ------------------------------------------------------------------------------------------------------------ the fixture
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(FIXTURE, allow_pickle=False))
    return _cache["z"]


def split_annos(z, prefix, keys):
    counts, names = z[f"{prefix}_counts"], z[f"{prefix}_name"]
    out, o = [], 0
    for n in counts:
        a = {"name": names[o:o + n].copy()}
        a.update({k: z[f"{prefix}_{k}"][o:o + n].copy() for k in keys})
        out.append(a)
        o += n
    return out


def load_set(name):
    """-> dict: gt_annos, dt_annos (float64 arrays, str names), classes, overlaps[metric] per-frame (dt, gt) lists, the reference's
    precision / recall / orientation [metric], thresholds / pr per metric in (class, difficulty, overlap) order, result, ret_dict"""
    key = ("set", name)
    if key in _cache:
        return _cache[key]
    z = fixture()
    gt, dt = split_annos(z, f"{name}_gt", GT_KEYS), split_annos(z, f"{name}_dt", DT_KEYS)
    meta = json.loads(str(z[f"{name}_meta"]))
    out = dict(gt_annos=gt, dt_annos=dt, classes=meta["classes"], compute_aos=meta["compute_aos"], result=str(z[f"{name}_result"]),
               ret_dict=dict(zip(meta["ret_keys"], z[f"{name}_ret_vals"].tolist())), overlaps={}, precision={}, recall={},
               orientation={}, thresholds={}, pr={})
    for metric in range(3):
        flat, o, blocks = z[f"{name}_ov{metric}"], 0, []
        for g, d in zip(gt, dt):
            n = len(g["name"]) * len(d["name"])
            blocks.append(flat[o:o + n].reshape(len(d["name"]), len(g["name"])))
            o += n
        out["overlaps"][metric] = blocks
        for k in ("precision", "recall", "orientation"):
            out[k][metric] = z[f"{name}_{k}{metric}"]
        lens, vals = z[f"{name}_thr_len{metric}"], z[f"{name}_thr{metric}"]
        cuts = np.concatenate([[0], np.cumsum(lens)])
        out["thresholds"][metric] = [vals[cuts[i]:cuts[i + 1]] for i in range(len(lens))]
        out["pr"][metric] = [z[f"{name}_pr{metric}"][cuts[i]:cuts[i + 1]] for i in range(len(lens))]
    _cache[key] = out
    return out


def metric_overlaps(classes, metric):
    """-> (K, num_class) rows of the official table for this metric"""
    return OVERLAP_TABLE[:, metric, :][:, list(classes)]


def restated(name, metric):
    """the restatement's eval_class on a fixture set from the RECORDED overlaps, computed once"""
    key = ("restated", name, metric)
    if key not in _cache:
        s = load_set(name)
        _cache[key] = eval_class(s["gt_annos"], s["dt_annos"], s["classes"], [0, 1, 2], metric, metric_overlaps(s["classes"], metric),
                                 s["overlaps"][metric], compute_aos=s["compute_aos"] and metric == 0)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ synthetic sets
SIZES = {"Car": (3.9, 1.5, 1.6), "Pedestrian": (0.8, 1.75, 0.6), "Cyclist": (1.76, 1.7, 0.6), "Van": (5.0, 2.2, 2.0),
         "Person_sitting": (0.8, 1.3, 0.6), "Truck": (8.0, 3.0, 2.5), "Tram": (15.0, 3.5, 2.5)}
FOCAL = 720.0


def make_object(name, x, hpx, ry, occluded=0, truncated=0.0, score=None):
    """a box of the class's size `hpx` pixels tall in the image (that fixes its depth), at lateral offset x"""
    l, h, w = SIZES[name]
    z = FOCAL * h / hpx
    u, bottom = 610.0 + FOCAL * x / z, 175.0 + FOCAL * 1.6 / z
    wpx = FOCAL * 0.7 * max(l, w) / z
    o = dict(name=name, bbox=[u - wpx / 2, bottom - hpx, u + wpx / 2, bottom], location=[x, 1.6, z], dimensions=[l, h, w],
             rotation_y=ry, alpha=ry - np.arctan2(x, z), occluded=occluded, truncated=truncated)
    if score is not None:
        o["score"] = score
    return o


def dontcare(bbox):
    return dict(name="DontCare", bbox=list(bbox), location=[-1000.0] * 3, dimensions=[-1.0] * 3, rotation_y=-10.0, alpha=-10.0,
                occluded=-1, truncated=-1.0)


def detection_of(obj, rng, score, shift=0.12, name=None, alpha=None):
    d = {k: (list(v) if isinstance(v, list) else v) for k, v in obj.items() if k not in ("occluded", "truncated")}
    d["name"] = name or obj["name"]
    d["location"] = [obj["location"][0] + rng.normal(0, shift), 1.6 + rng.normal(0, 0.04), obj["location"][2] + rng.normal(0, shift)]
    d["dimensions"] = [v * rng.uniform(0.94, 1.06) for v in obj["dimensions"]]
    d["rotation_y"] = obj["rotation_y"] + rng.normal(0, 0.04)
    x0, y0, x1, y1 = obj["bbox"]
    e = rng.uniform(-0.04, 0.04, 4) * [x1 - x0, y1 - y0, x1 - x0, y1 - y0]
    d["bbox"] = [x0 + e[0], y0 + e[1], x1 + e[2], y1 + e[3]]
    d["alpha"] = obj["alpha"] + rng.normal(0, 0.15) if alpha is None else alpha
    d["score"] = score
    return d


def to_anno(objs, keys):
    a = {"name": np.array([o["name"] for o in objs], dtype="<U16")}
    for k in keys:
        width = {"bbox": 4, "location": 3, "dimensions": 3}.get(k)
        vals = np.array([o[k] for o in objs], np.float64)
        a[k] = vals.reshape(len(objs), width) if width else vals.reshape(len(objs))
    return a


def margin_problems(blocks, scores, floor=1e-3, allow_pairs=()):
    """violations of the decision margins for one frame: blocks = list of (dt, gt) overlap arrays (every metric and the dt x
    DontCare block), scores (dt).  allow_pairs: det row pairs that are duplicates on purpose."""
    bad = []
    for b, ov in enumerate(blocks):
        for t in (0.7, 0.5, 0.25):
            close = (np.abs(ov - t) <= 1e-3) & (ov != 0)
            if close.any():
                bad.append(f"block {b}: an overlap within 1e-3 of {t}")
        if ((ov != 0) & (np.abs(ov) < floor)).any():
            bad.append(f"block {b}: a non-zero overlap below {floor}")
        for i in range(ov.shape[1]):
            rows = np.nonzero(ov[:, i] > 0)[0]
            for a in range(len(rows)):
                for c in range(a + 1, len(rows)):
                    pair = (int(rows[a]), int(rows[c]))
                    if pair not in allow_pairs and abs(ov[rows[a], i] - ov[rows[c], i]) <= 1e-3:
                        bad.append(f"block {b} gt {i}: dets {pair} have overlaps closer than 1e-3")
    s = np.asarray(scores)
    for a in range(len(s)):
        for c in range(a + 1, len(s)):
            if s[a] == s[c] and (a, c) not in allow_pairs:
                bad.append(f"dets {a} and {c} have equal scores")
    return bad
