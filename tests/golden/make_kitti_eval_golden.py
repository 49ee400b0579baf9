"""Generates tests/golden/kitti_eval_ref.npz from the REFERENCE ITSELF: its own get_official_eval_result
(pcdet/datasets/kitti/kitti_object_eval_python/eval.py), loaded from its file and run in plain Python on the CPU.  Runs only where the
reference checkout is (default /root/reference, or $LIDAR_REFERENCE) and oracle/_build is built.

How the reference is loaded: numba is not installed, so eval.py and rotate_iou.py are loaded under a stand-in `numba` module whose
`jit` and `cuda.jit` are identity decorators, and eval.py's rotate_iou_gpu_eval (numba.cuda) is replaced by
oracle.c_oracle.rotate_iou_eval, the C restatement of its numba source: the rotated IoU stays "unpinned" as everywhere in this project,
everything around it is the reference's own code.  Every anno array is float64, so that numba-versus-Python typing of mixed dtypes
cannot matter.  get_thresholds and fused_compute_statistics are wrapped to RECORD what they return (thresholds, the tp / fp / fn /
similarity table) next to the curves.

Recorded per set: the annos, the per-frame overlaps eval_class saw for the three metrics, precision / recall / orientation per
metric, thresholds and pr tables, the result string and ret_dict.  Also the output of lidar_rotate_iou_eval at the commit before the
AP evaluation was added, on the inputs of tests/test_gpu_roi_pool.py::test_kitti_eval_rotate_iou_matches_oracle (riou_*; taken from
a GPU run, passed in with --riou FILE, else kept from the existing fixture).

Sets
  main    24 frames, classes Car / Pedestrian / Cyclist, AOS on.  Each of the following is ASSERTED below:
            a frame with no gt, one with no dt, one with neither
            DontCare boxes that absorb otherwise-false-positive dets (metric 0)
            a Van matched by a Car det and a Person_sitting matched by a Pedestrian det
            a gt ignored by each of occlusion, truncation and height at easy but valid at hard
            a det below the height limit that is the only match of a gt (the matcher's third branch)
            a det below the height limit and a regular det over the same gt, the ignored one at the lower row
            two dets over one gt where the higher score has the lower overlap (pass 1 and pass 2 choose differently)
            two identical duplicate dets (equal overlap, equal score): the lowest row wins in both passes
            a det of another class
            Cyclist has no valid gt at easy: no thresholds, zero curves
            more than 41 matched scores for Car, so get_thresholds skips
  noaos   4 frames whose first dt alpha is -10: AOS off

Decision margins, ASSERTED for every frame so that fp32 reordering on the device cannot flip an outcome: every same-frame overlap of
every metric (and every dt x DontCare overlap) lies more than 1e-3 from 0.7, 0.5 and 0.25 or is exactly 0; apart from the duplicated
pair no two dets overlapping one gt have overlaps closer than 1e-3, and no two dets of a frame have equal scores; (ours, not the
issue's) a non-zero overlap is at least 1e-3, so "exactly 0" means disjoint boxes.  A frame is drawn again until it meets them;
nothing is excluded afterwards.

Usage:  python tests/golden/make_kitti_eval_golden.py [--riou FILE.npz]
"""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refkitti_eval"
OUT = os.path.join(HERE, "kitti_eval_ref.npz")

import _kitti_eval_np as ke  # noqa: E402
from oracle import c_oracle  # noqa: E402

RECORD = {"thresholds": [], "pr": []}


def load_reference():
    """-> the reference's eval module, rotate_iou_gpu_eval replaced and the two recorders installed"""
    def identity_jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn

    numba = types.ModuleType("numba")
    numba.jit = identity_jit
    numba.cuda = types.ModuleType("numba.cuda")
    numba.cuda.jit = identity_jit
    saved = {k: sys.modules.get(k) for k in ("numba", "numba.cuda")}
    sys.modules["numba"], sys.modules["numba.cuda"] = numba, numba.cuda
    try:
        folder = os.path.join(REF, "pcdet", "datasets", "kitti", "kitti_object_eval_python")
        pkg = types.ModuleType(PKG)
        pkg.__path__ = [folder]
        sys.modules[PKG] = pkg
        mods = {}
        for name in ("rotate_iou", "eval"):
            spec = importlib.util.spec_from_file_location(f"{PKG}.{name}", os.path.join(folder, f"{name}.py"))
            mods[name] = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mods[name]
            spec.loader.exec_module(mods[name])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    ev = mods["eval"]
    ev.rotate_iou_gpu_eval = lambda boxes, query, criterion=-1: c_oracle.rotate_iou_eval(
        np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(query, np.float32), criterion)
    get_thresholds, fused = ev.get_thresholds, ev.fused_compute_statistics

    def rec_thresholds(scores, num_gt, num_sample_pts=41):
        out = get_thresholds(scores, num_gt, num_sample_pts)
        RECORD["thresholds"].append(np.array(out, np.float64))
        return out

    def rec_fused(overlaps, pr, *args, **kwargs):
        fused(overlaps, pr, *args, **kwargs)
        RECORD["pr"].append(pr)          # the same array for every part of a configuration: read after eval_class returns

    ev.get_thresholds, ev.fused_compute_statistics = rec_thresholds, rec_fused
    return ev


# ------------------------------------------------------------------------------------------------------------ frames
def frame_blocks(ev, gts, dts):
    """the (dt, gt) overlap blocks of one frame for the three metrics and dt x DontCare, as the reference computes them"""
    g, d = ke.to_anno(gts, ke.GT_KEYS), ke.to_anno(dts, ke.DT_KEYS)
    if not len(gts) or not len(dts):
        return []
    blocks = [ev.calculate_iou_partly([d], [g], metric, 100)[0][0] for metric in range(3)]
    dc = g["bbox"][g["name"] == "DontCare"]
    if len(dc):
        blocks.append(ev.image_box_overlap(d["bbox"], dc, 0))
    return blocks


def draw_frame(ev, rng, builder, allow_pairs=()):
    for _ in range(2000):
        gts, dts = builder(rng)
        bad = ke.margin_problems(frame_blocks(ev, gts, dts), [d["score"] for d in dts], allow_pairs=allow_pairs)
        if not bad:
            return gts, dts
    raise AssertionError(f"no draw meets the margins: {bad}")


def lanes(rng, n):
    """n distinct lateral offsets, 4 m apart, so that only the intended boxes overlap on the ground"""
    return [float(x) + rng.uniform(-0.3, 0.3) for x in rng.permutation(np.arange(-14, 15, 4))[:n]]


def regular(rng):
    """three or four cars (all taller than 40 px), pedestrians and a cyclist that is too small for easy, most of them detected"""
    xs = lanes(rng, 8)
    gts = [ke.make_object("Car", xs[i], rng.uniform(44, 90), rng.uniform(-np.pi, np.pi)) for i in range(int(rng.integers(3, 5)))]
    gts += [ke.make_object("Pedestrian", xs[4], rng.uniform(45, 80), rng.uniform(-np.pi, np.pi)),
            ke.make_object("Pedestrian", xs[5], rng.uniform(27, 39), rng.uniform(-np.pi, np.pi)),
            ke.make_object("Cyclist", xs[6], rng.uniform(27, 39), rng.uniform(-np.pi, np.pi))]
    dts = [ke.detection_of(g, rng, rng.uniform(0.05, 1.0), shift=rng.choice([0.05, 0.12, 0.3])) for g in gts if rng.random() < 0.9]
    ghost = ke.make_object(str(rng.choice(["Car", "Pedestrian", "Cyclist"])), xs[7], rng.uniform(30, 70), rng.uniform(-3, 3))
    dts.append(ke.detection_of(ghost, rng, rng.uniform(0.05, 0.6)))                     # a false positive
    order = rng.permutation(len(dts))
    return gts, [dts[i] for i in order]


def exact_det(obj, score, dx=0.0, dpx=0.0, name=None):
    """the gt's own box as a det, moved dx metres sideways on the ground and dpx pixels in the image"""
    d = {k: (list(v) if isinstance(v, list) else v) for k, v in obj.items() if k not in ("occluded", "truncated")}
    d["location"][0] += dx
    d["bbox"] = [d["bbox"][0] + dpx, d["bbox"][1], d["bbox"][2] + dpx, d["bbox"][3]]
    d.update(name=name or obj["name"], alpha=obj["alpha"] + 0.1, score=score)
    return d


def only_dets(rng):
    return [], [ke.detection_of(ke.make_object("Car", x, 60, 0.3), rng, s) for x, s in zip(lanes(rng, 2), (0.8, 0.4))]


def only_gts(rng):
    xs = lanes(rng, 2)
    return [ke.make_object("Car", xs[0], 70, 1.0), ke.make_object("Pedestrian", xs[1], 50, -2.0)], []


def empty(rng):
    return [], []


def dontcare_frame(rng):
    """two Car dets and a Pedestrian det without a gt whose image boxes lie inside DontCare regions, and a matched car"""
    xs = lanes(rng, 4)
    car = ke.make_object("Car", xs[0], 70, rng.uniform(-3, 3))
    ghosts = [ke.make_object("Car", xs[1], 50, 0.2), ke.make_object("Car", xs[2], 48, -1.0), ke.make_object("Pedestrian", xs[3], 45, 0.5)]
    dts = [exact_det(car, 0.9, 0.05, 2.0)] + [ke.detection_of(g, rng, s) for g, s in zip(ghosts, (0.7, 0.55, 0.45))]
    regions = []
    for d in dts[1:]:
        x0, y0, x1, y1 = d["bbox"]
        regions.append(ke.dontcare([x0 - rng.uniform(5, 30), y0 - rng.uniform(5, 20), x1 + rng.uniform(5, 30), y1 + rng.uniform(5, 20)]))
    return [car] + regions, dts


def neighbours(rng):
    """a Van under a Car det, a Person_sitting under a Pedestrian det, dets of other classes, a Truck and a Tram"""
    xs = lanes(rng, 6)
    van, sit = ke.make_object("Van", xs[0], 80, 0.4), ke.make_object("Person_sitting", xs[1], 45, 1.2)
    car, truck, tram = ke.make_object("Car", xs[2], 60, -0.7), ke.make_object("Truck", xs[3], 90, 0.1), ke.make_object("Tram", xs[4], 80, 1.5)
    gts = [van, sit, car, truck, tram]
    dts = [exact_det(van, 0.85, 0.08, 3.0, name="Car"), exact_det(sit, 0.6, 0.02, 1.0, name="Pedestrian"),
           ke.detection_of(car, rng, 0.75, name="Cyclist", shift=0.05),                # another class over a Car gt
           exact_det(car, 0.5, 0.06, 2.0), ke.detection_of(truck, rng, 0.65, shift=0.1),
           ke.detection_of(tram, rng, 0.35, name="tram", shift=0.1)]
    return gts, dts


def hard_only(rng):
    """cars ignored at easy by occlusion, by truncation and by height, all valid at hard; each detected"""
    xs = lanes(rng, 3)
    gts = [ke.make_object("Car", xs[0], 70, 0.3, occluded=1), ke.make_object("Car", xs[1], 65, -1.2, truncated=0.4),
           ke.make_object("Car", xs[2], 33, 2.0)]
    return gts, [exact_det(g, s, dx, 1.5) for g, s, dx in zip(gts, (0.82, 0.64, 0.47), (0.04, 0.07, 0.1))]


def squeeze(det, obj, height):
    """the det's image box on the gt's columns, `height` pixels tall inside the gt's rows"""
    x0, y0, x1, y1 = obj["bbox"]
    det["bbox"] = [x0, y1 - height - 1.0, x1, y1 - 1.0]
    return det


def small_dets(rng):
    """pedestrian gts 30 px tall (valid at moderate and hard).  gt 0: its only det is 24 px tall (ignored_det 1 everywhere, image IoU
    0.8): branch three.  gt 1: a 24 px det at the lower row and a regular det after it: the ignored assignment is overwritten."""
    xs = lanes(rng, 2)
    a, b = ke.make_object("Pedestrian", xs[0], 30, 0.5), ke.make_object("Pedestrian", xs[1], 30, -0.8)
    dts = [squeeze(exact_det(a, 0.7, 0.02), a, 24.0), squeeze(exact_det(b, 0.9, 0.02), b, 24.0), squeeze(exact_det(b, 0.6, 0.05), b, 28.5)]
    return [a, b], dts


def two_over_one(rng):
    """gt 0: det 0 has the higher score and the lower overlap, det 1 the reverse.  gt 1: dets 2 and 3 are identical duplicates."""
    xs = lanes(rng, 3)
    a, b, c = ke.make_object("Car", xs[0], 70, 0.2), ke.make_object("Car", xs[1], 60, -2.5), ke.make_object("Car", xs[2], 55, 1.1)
    far, near, dup = exact_det(a, 0.95, 0.16, 6.0), exact_det(a, 0.55, 0.03, 1.0), exact_det(b, 0.77, 0.05, 2.0)
    return [a, b, c], [far, near, dup, exact_det(b, 0.77, 0.05, 2.0), exact_det(c, 0.4, 0.07, 3.0)]


MAIN = [regular] * 4 + [only_dets, regular, only_gts, regular, empty, dontcare_frame, regular, neighbours, regular, hard_only, regular,
                        small_dets, regular, two_over_one] + [regular] * 6
DUP_PAIRS = {two_over_one: ((2, 3),)}


def build_set(ev, seed, builders, alpha_off=False):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for b in builders:
        g, d = draw_frame(ev, rng, b, DUP_PAIRS.get(b, ()))
        if alpha_off:
            for x in d:
                x["alpha"] = -10.0
        gts.append(ke.to_anno(g, ke.GT_KEYS))
        dts.append(ke.to_anno(d, ke.DT_KEYS))
    return gts, dts


# ------------------------------------------------------------------------------------------------------------ run and record
def run_set(ev, name, gts, dts, classes, out):
    for key in RECORD:
        del RECORD[key][:]
    detail = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        result, ret = ev.get_official_eval_result(gts, dts, classes, PR_detail_dict=detail)
    aos = "aos" in detail
    for prefix, annos, keys in ((f"{name}_gt", gts, ke.GT_KEYS), (f"{name}_dt", dts, ke.DT_KEYS)):
        out[f"{prefix}_counts"] = np.array([len(a["name"]) for a in annos], np.int64)
        out[f"{prefix}_name"] = np.concatenate([a["name"] for a in annos]).astype("<U16")
        for k in keys:
            out[f"{prefix}_{k}"] = np.concatenate([a[k] for a in annos], 0).astype(np.float64)
    n_cfg = len(classes) * 3 * 2
    assert len(RECORD["thresholds"]) == 3 * n_cfg and len(RECORD["pr"]) == 3 * n_cfg, "one part per configuration is assumed"
    class_ids = [ke.DISPLAY.index(c) for c in classes]
    for metric in range(3):
        blocks = ev.calculate_iou_partly(dts, gts, metric, 100)[0]
        out[f"{name}_ov{metric}"] = np.concatenate([b.reshape(-1) for b in blocks]).astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            curves = ev.eval_class(gts, dts, class_ids, [0, 1, 2], metric, ke.OVERLAP_TABLE[:, :, class_ids], aos and metric == 0)
        for k in ("precision", "recall", "orientation"):
            out[f"{name}_{k}{metric}"] = curves[k]
        thr = RECORD["thresholds"][metric * n_cfg:(metric + 1) * n_cfg]
        pr = RECORD["pr"][metric * n_cfg:(metric + 1) * n_cfg]
        out[f"{name}_thr_len{metric}"] = np.array([len(t) for t in thr], np.int64)
        out[f"{name}_thr{metric}"] = np.concatenate(thr) if thr else np.zeros(0)
        out[f"{name}_pr{metric}"] = np.concatenate([p.reshape(-1, 4) for p in pr], 0)
    assert np.array_equal(detail["bbox"], out[f"{name}_precision0"]) and np.array_equal(detail["3d"], out[f"{name}_precision2"])
    out[f"{name}_result"] = np.array(result)
    out[f"{name}_ret_vals"] = np.array([float(v) for v in ret.values()], np.float64)
    out[f"{name}_meta"] = np.array(json.dumps(dict(classes=class_ids, compute_aos=aos, ret_keys=list(ret.keys()))))
    print(name, len(gts), "frames", sum(len(a["name"]) for a in gts), "gt", sum(len(a["name"]) for a in dts), "dt, aos", aos)
    print(result)


def check_cases(ev, gts, dts):
    """the main set holds what the docstring lists (frame numbers as in MAIN)"""
    ng, nd = [len(a["name"]) for a in gts], [len(a["name"]) for a in dts]
    assert any(g == 0 and d > 0 for g, d in zip(ng, nd)) and any(g > 0 and d == 0 for g, d in zip(ng, nd))
    assert any(g == 0 and d == 0 for g, d in zip(ng, nd))

    def stats(f, cls, diff, metric, mo, thresh, dc=True):
        _, ig, idt, dcb = ev.clean_data(gts[f], dts[f], cls, diff)
        dcb = np.stack(dcb, 0) if len(dcb) and dc else np.zeros((0, 4))
        ov = ev.calculate_iou_partly([dts[f]], [gts[f]], metric, 100)[0][0]
        gd = np.concatenate([gts[f]["bbox"], gts[f]["alpha"][:, None]], 1)
        dd = np.concatenate([dts[f]["bbox"], dts[f]["alpha"][:, None], dts[f]["score"][:, None]], 1)
        return ev.compute_statistics_jit(ov, gd, dd, np.array(ig), np.array(idt), dcb, metric, mo, thresh, thresh is not None), ig, idt, ov

    f = MAIN.index(dontcare_frame)
    with_dc, without = stats(f, 0, 1, 0, 0.7, 0.0)[0], stats(f, 0, 1, 0, 0.7, 0.0, dc=False)[0]
    assert with_dc[1] == 0 and without[1] == 2, "the DontCare boxes absorb two Car false positives"
    assert stats(f, 1, 1, 0, 0.5, 0.0)[0][1] == 0 and stats(f, 1, 1, 0, 0.5, 0.0, dc=False)[0][1] == 1
    f = MAIN.index(neighbours)
    for cls, metric, mo in ((0, 0, 0.7), (0, 1, 0.7), (0, 2, 0.7), (1, 0, 0.5), (1, 1, 0.5), (1, 2, 0.5)):
        (tp, fp, fn, _, _), ig, idt, ov = stats(f, cls, 1, metric, mo, 0.0)
        row = 0 if cls == 0 else 1
        assert ig[row] == 1 and idt[row] == 0 and ov[row, row] > mo and fp == 0, "the neighbour class absorbs the det uncounted"
    assert -1 in stats(f, 0, 1, 0, 0.7, 0.0)[2] and (gts[f]["name"] == "Tram").any() and (dts[f]["name"] == "tram").any()
    f = MAIN.index(hard_only)
    assert [ev.clean_data(gts[f], dts[f], 0, d)[1] for d in (0, 1, 2)] == [[1, 1, 1], [0, 1, 0], [0, 0, 0]]
    f = MAIN.index(small_dets)
    for metric, mo in ((0, 0.5), (1, 0.5), (2, 0.5), (1, 0.25), (2, 0.25)):
        (tp, fp, fn, _, _), ig, idt, ov = stats(f, 1, 1, metric, mo, 0.0)
        assert ig == [0, 0] and idt == [1, 1, 0] and ov[0, 0] > mo and ov[1, 1] > mo and ov[2, 1] > mo
        assert (tp, fp, fn) == (1, 0, 0), "gt 0 is assigned to the ignored det (no fn, no tp), gt 1 goes to the regular det"
    f = MAIN.index(two_over_one)
    for metric, mo in ((0, 0.7), (1, 0.7), (2, 0.7), (1, 0.5), (2, 0.5)):
        (_, _, _, _, emitted), ig, idt, ov = stats(f, 0, 0, metric, mo, None)
        assert ov[0, 0] > mo and ov[1, 0] > ov[0, 0] + 1e-3 and dts[f]["score"][0] > dts[f]["score"][1]
        assert emitted[0] == dts[f]["score"][0], "pass 1 takes the higher score"
        assert ov[2, 1] == ov[3, 1] > mo and dts[f]["score"][2] == dts[f]["score"][3]
        (tp, fp, fn, _, _) = stats(f, 0, 0, metric, mo, 0.0)[0]
        assert (tp, fp, fn) == (3, 2, 0), "pass 2 takes the larger overlap; the other det and one duplicate are false positives"
    valid = [[sum(ev.clean_data(g, d, c, diff)[0] for g, d in zip(gts, dts)) for diff in (0, 1, 2)] for c in (0, 1, 2)]
    assert valid[2][0] == 0 and valid[2][1] > 0 and valid[2][2] > 0, valid


def check_recorded(out, name):
    """cyclist at easy has no thresholds and zero curves; a Car configuration has more than 41 matched scores"""
    for metric in range(3):
        lens = out[f"{name}_thr_len{metric}"].reshape(3, 3, 2)
        assert (lens[2, 0] == 0).all() and not out[f"{name}_precision{metric}"][2, 0].any()
        assert (lens[2, 1:] > 0).all() and lens.max() <= 41
        pr = out[f"{name}_pr{metric}"]
        cuts = np.concatenate([[0], np.cumsum(lens.reshape(-1))])
        first_car_hard = pr[cuts[2 * 2 + 1]:cuts[2 * 2 + 2]]            # class 0, difficulty 2, overlap row 1
        assert first_car_hard[-1, 0] > 41 and len(first_car_hard) < first_car_hard[-1, 0], "get_thresholds must skip scores"


def main():
    ev = load_reference()
    out = {}
    gts, dts = build_set(ev, 20250, MAIN)
    check_cases(ev, gts, dts)
    run_set(ev, "main", gts, dts, ["Car", "Pedestrian", "Cyclist"], out)
    check_recorded(out, "main")
    assert json.loads(str(out["main_meta"]))["compute_aos"]
    gts2, dts2 = build_set(ev, 7, [regular, neighbours, regular, hard_only], alpha_off=True)
    run_set(ev, "noaos", gts2, dts2, ["Car", "Pedestrian"], out)
    assert not json.loads(str(out["noaos_meta"]))["compute_aos"] and "aos" not in str(out["noaos_result"])
    riou = sys.argv[sys.argv.index("--riou") + 1] if "--riou" in sys.argv else OUT
    out.update({k: v for k, v in np.load(riou).items() if k.startswith("riou_")})
    assert len([k for k in out if k.startswith("riou_out_")]) == 4, "the recorded lidar_rotate_iou_eval outputs are missing"
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
