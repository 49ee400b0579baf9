"""KITTI AP evaluation on the GPU (lidardetection_amd/kitti_eval.py, csrc/kitti_eval.hip, the eval.py mirror) against the reference's
own eval.py (tests/golden/kitti_eval_ref.npz, written by tests/golden/make_kitti_eval_golden.py with asserted decision margins) and
against the numpy restatement of tests/_kitti_eval_np.py, which tests/test_kitti_eval_host.py pins to that fixture.

Tolerances: image overlaps 1e-12 (the same fp64 expression); rotated overlaps 1e-4 (the project's stated parity for fp32 geometry),
exact zeros exactly zero; matched scores, thresholds and tp / fp / fn exactly; precision and recall 1e-12, AOS and mAP 1e-9 (fp64
sums of at most a few thousand terms in [0, 1])."""
import numpy as np
import pytest
import torch

import _kitti_eval_np as ke
from lidardetection_amd import _lib, kitti_eval
from lidardetection_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_mirror
from lidardetection_amd.pcdet.datasets.kitti.kitti_object_eval_python.rotate_iou import rotate_iou_gpu_eval

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETS = ("main", "noaos")
_packed = {}


def packed_set(name):
    if name not in _packed:
        s = ke.load_set(name)
        _packed[name] = kitti_eval.pack(s["gt_annos"], s["dt_annos"], DEV)
    return _packed[name]


# ------------------------------------------------------------------------------------------------ (a) overlaps
@pytest.mark.parametrize("name", SETS)
def test_overlaps(name):
    s, p = ke.load_set(name), packed_set(name)
    got = [p.overlap_blocks(metric) for metric in range(3)]
    dc = p.overlap_blocks(0, 0)
    seen = 0
    for f, (g, d) in enumerate(zip(s["gt_annos"], s["dt_annos"])):
        assert got[0][f].shape == (len(d["name"]), len(g["name"])) and got[0][f].dtype == np.float64
        assert np.abs(got[0][f] - ke.image_overlap(d["bbox"], g["bbox"])).max(initial=0) <= 1e-12
        assert np.abs(dc[f] - ke.image_overlap(d["bbox"], g["bbox"], 0)).max(initial=0) <= 1e-12
        for metric in (1, 2):
            want = s["overlaps"][metric][f]
            print(name, f, metric, float(np.abs(got[metric][f] - want).max(initial=0)))
            assert np.abs(got[metric][f] - want).max(initial=0) <= 1e-4
            assert np.array_equal(got[metric][f] == 0, want == 0)
            assert np.array_equal(got[metric][f], got[metric][f].astype(np.float32))        # fp32 values, as the reference casts them
            seen += int((want > 0).sum())
    assert seen > 10


def test_mirror_overlap_functions():
    s = ke.load_set("main")
    f = max(range(24), key=lambda i: len(s["gt_annos"][i]["name"]) * len(s["dt_annos"][i]["name"]))
    g, d = s["gt_annos"][f], s["dt_annos"][f]
    for criterion in (-1, 0, 1):
        assert np.abs(kitti_mirror.image_box_overlap(d["bbox"], g["bbox"], criterion) - ke.image_overlap(d["bbox"], g["bbox"], criterion)).max() <= 1e-12
    box7 = lambda a: np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], 1)  # noqa: E731
    d3 = kitti_mirror.d3_box_overlap(box7(d), box7(g))
    assert d3.dtype == np.float32 and np.abs(d3 - s["overlaps"][2][f]).max() <= 1e-4
    bev = kitti_mirror.bev_box_overlap(box7(d)[:, [0, 2, 3, 5, 6]], box7(g)[:, [0, 2, 3, 5, 6]])
    assert np.abs(bev - s["overlaps"][1][f]).max() <= 1e-4
    for metric in range(3):
        blocks, parted, n_first, n_second = kitti_mirror.calculate_iou_partly(s["dt_annos"], s["gt_annos"], metric, num_parts=5)
        assert len(parted) == 6 and n_first.tolist() == [len(a["name"]) for a in s["dt_annos"]] and len(n_second) == 24
        assert all(np.abs(b - w).max(initial=0) <= 1e-4 for b, w in zip(blocks, s["overlaps"][metric]))
        assert sum(p.shape[0] for p in parted) == n_first.sum() and sum(p.shape[1] for p in parted) == n_second.sum()
        assert sum(float(p.sum()) for p in parted) == pytest.approx(sum(float(b.sum()) for b in blocks))


# ------------------------------------------------------------------------------------------------ (b) matching
def compare_with_restatement(p, gts, dts, classes, diffs, metric, min_overlaps, aos):
    """device eval_class against the restatement run on the device's own overlaps"""
    got = p.eval_class(classes, diffs, metric, min_overlaps, aos, details=True)
    want = ke.eval_class(gts, dts, classes, diffs, metric, min_overlaps, p.overlap_blocks(metric), aos)
    C, D, K = len(classes), len(diffs), len(min_overlaps)
    matched = got["matched"].cpu().numpy().reshape(C, D, K, p.total_gt)
    starts = np.concatenate([[0], np.cumsum(p.gt_counts)])
    nthr, thr, counts = (got[k].cpu().numpy() for k in ("num_thresholds", "thresholds", "counts"))
    assert np.array_equal(got["num_valid_gt"].cpu().numpy(), want["num_valid_gt"])
    for m in range(C):
        for l in range(D):
            for k in range(K):
                exp = np.full(p.total_gt, -np.inf)
                for f, emitted in enumerate(want["matched"][m][l][k]):
                    for row, score in emitted:
                        exp[starts[f] + row] = score
                assert np.array_equal(matched[m, l, k], exp)
                assert thr[m, l, k, :nthr[m, l, k]].tolist() == want["thresholds"][m][l][k]
    assert np.array_equal(counts, want["counts"])
    for key, tol in (("precision", 1e-12), ("recall", 1e-12), ("orientation", 1e-9)):
        assert got[key].shape == (C, D, K, 41)
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
        assert np.nanmax(np.abs(got[key] - want[key]), initial=0) <= tol, key
    return got, want


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", SETS)
def test_matching_on_fixture(name, metric):
    s, p = ke.load_set(name), packed_set(name)
    aos = s["compute_aos"] and metric == 0
    got, want = compare_with_restatement(p, s["gt_annos"], s["dt_annos"], s["classes"], [0, 1, 2], metric,
                                         ke.metric_overlaps(s["classes"], metric), aos)
    # the device's overlaps lead to the reference's own curves: the margins keep every decision
    assert np.abs(got["precision"] - s["precision"][metric]).max() <= 1e-12
    assert np.abs(got["recall"] - s["recall"][metric]).max() <= 1e-12
    assert np.abs(got["orientation"] - s["orientation"][metric]).max() <= 1e-9
    n = 0
    for m in range(len(s["classes"])):
        for l in range(3):
            for k in range(2):
                assert want["thresholds"][m][l][k] == s["thresholds"][metric][n].tolist()
                n += 1


# ------------------------------------------------------------------------------------------------ (c) end to end, (e) twice
@pytest.mark.parametrize("name", SETS)
def test_official_result_matches_reference_and_repeats(name):
    s = ke.load_set(name)
    names = [ke.DISPLAY[c] for c in s["classes"]]
    runs = []
    for _ in range(2):
        detail = {}
        result, ret = kitti_mirror.get_official_eval_result(s["gt_annos"], s["dt_annos"], names, PR_detail_dict=detail)
        runs.append((result, ret, detail))
    result, ret, detail = runs[0]
    assert result == s["result"]
    assert list(ret) == list(s["ret_dict"])
    assert all(abs(float(ret[k]) - s["ret_dict"][k]) <= 1e-9 for k in ret)
    assert set(detail) == {"bbox", "bev", "3d"} | ({"aos"} if s["compute_aos"] else set())
    for key, metric in (("bbox", 0), ("bev", 1), ("3d", 2)):
        assert detail[key].shape == (len(names), 3, 2, 41) and np.abs(detail[key] - s["precision"][metric]).max() <= 1e-12
    if s["compute_aos"]:
        assert np.abs(detail["aos"] - s["orientation"][0]).max() <= 1e-9
    assert runs[1][0] == result
    assert all(np.array_equal(detail[k], runs[1][2][k]) for k in detail)                 # bit for bit
    assert all(np.array_equal(np.float64(ret[k]), np.float64(runs[1][1][k])) for k in ret)
    single = kitti_mirror.get_official_eval_result(s["gt_annos"], s["dt_annos"], "Car")[0]      # one class, not in a list
    assert single == result[:len(single)]


def test_eval_class_mirror_signature():
    s = ke.load_set("main")
    ret = kitti_mirror.eval_class(s["gt_annos"], s["dt_annos"], [0, 1, 2], [0, 1, 2], 2, ke.OVERLAP_TABLE[:, :, [0, 1, 2]])
    assert set(ret) == {"recall", "precision", "orientation"} and not ret["orientation"].any()
    assert np.abs(ret["recall"] - s["recall"][2]).max() <= 1e-12
    maps = kitti_mirror.do_eval(s["gt_annos"], s["dt_annos"], [0, 1, 2], ke.OVERLAP_TABLE[:, :, [0, 1, 2]], True)
    assert len(maps) == 8 and np.abs(maps[6] - ke.map_r40(s["precision"][2])).max() <= 1e-9
    assert np.abs(maps[0] - ke.map_r11(s["precision"][0])).max() <= 1e-9 and np.abs(maps[7] - ke.map_r40(s["orientation"][0])).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ (d) shapes
def synthetic_frame(rng, n_gt, n_dt, n_over=None):
    """gts on a grid, far apart in the image and on the ground; every det is one gt's box moved sideways by a share of its width that
    keeps the IoU (w - s) / (w + s) of all three metrics more than 2e-3 from 0.7, 0.5, 0.25 and from the other dets of that gt.  Only
    n_over dets (default: all, at random rows) lie over a gt, the others over nothing: a gt cannot hold hundreds of dets 1e-3 apart.  Every
    tenth det is a Van-sized "Cyclist", every seventh det is 20 px tall (ignored), every ninth gt is a Van, every eleventh occluded."""
    gts, taken = [], {}
    for i in range(n_gt):
        col, row = i % 16, i // 16
        l, h, w = ke.SIZES["Car"]
        z = 20.0 + 12.0 * row
        x = -60.0 + 8.0 * col
        u, v = 100.0 + 110.0 * col, 100.0 + 90.0 * row
        gts.append(dict(name="Van" if i % 9 == 8 else "Car", bbox=[u, v, u + 60.0, v + 50.0], location=[x, 1.6, z],
                        dimensions=[l, h, w], rotation_y=0.0, alpha=float(rng.uniform(-3, 3)), occluded=int(i % 11 == 10),
                        truncated=0.0))
    dts = []
    scores = rng.permutation(n_dt * 4)[:n_dt] / (n_dt * 4.0) + 0.01
    over = set(rng.permutation(n_dt)[:n_dt if n_over is None else n_over].tolist())
    for j in range(n_dt):
        if j not in over:
            l, h, w = ke.SIZES["Car"]
            u, v = 100.0 + 110.0 * (j % 16), 2000.0 + 90.0 * (j // 16)
            dts.append(dict(name="Car", bbox=[u, v, u + 60.0, v + 50.0], location=[-60.0 + 8.0 * (j % 16), 1.6, 500.0 + 12.0 * (j // 16)],
                            dimensions=[l, h, w], rotation_y=0.0, alpha=0.0, score=float(scores[j])))
            continue
        i = int(rng.integers(0, n_gt))
        while True:
            share = float(rng.uniform(0.0, 0.7))
            iou = (1 - share) / (1 + share)
            short = 1200.0 * (1 - share) / (4200.0 - 1200.0 * (1 - share))        # a 60 x 20 box inside the shifted 60 x 50 one
            vals = [iou, short] if j % 7 == 6 else [iou]
            if all(abs(v - t) > 2e-3 for v in vals for t in (0.7, 0.5, 0.25)) and \
                    all(abs(v - o) > 2e-3 for v in vals for o in taken.get(i, [])):
                break
        taken.setdefault(i, []).extend(vals)
        g = gts[i]
        u0, v0, u1, v1 = g["bbox"]
        bbox = [u0 + 60.0 * share, v0, u1 + 60.0 * share, v1]
        if j % 7 == 6:
            bbox[1], bbox[3] = v0 + 10.0, v0 + 30.0
        dts.append(dict(name="Cyclist" if j % 10 == 9 else "Car", bbox=bbox,
                        location=[g["location"][0] + g["dimensions"][0] * share, 1.6, g["location"][2]], dimensions=list(g["dimensions"]),
                        rotation_y=0.0, alpha=float(rng.uniform(-3, 3)), score=float(scores[j])))
    return ke.to_anno(gts, ke.GT_KEYS), ke.to_anno(dts, ke.DT_KEYS)


def check_margins(p, dup=()):
    for metric in range(3):
        for f, block in enumerate(p.overlap_blocks(metric)):
            bad = ke.margin_problems([block], [], allow_pairs=dup)
            assert not bad, (metric, f, bad[:3])


@pytest.mark.parametrize("n_gt,n_dt,frames", [(70, 130, 1), (2, 1024, 1), (1, 1, 65)])
def test_shapes_against_restatement(n_gt, n_dt, frames):
    rng = np.random.default_rng(1000 + n_dt)
    annos = [synthetic_frame(rng, n_gt, n_dt, 60 if n_dt == 1024 else None) for _ in range(frames)]
    gts, dts = [a[0] for a in annos], [a[1] for a in annos]
    if frames > 1:                      # distinct scores over the set, so that the sorted order has no ties
        for f, d in enumerate(dts):
            d["score"] = d["score"] * 0 + (f + 1) / (frames + 2.0)
    p = kitti_eval.pack(gts, dts, DEV)
    assert (p.max_gt, p.max_dt, p.frames) == (n_gt, n_dt, frames)
    check_margins(p)
    for metric, aos in ((0, True), (2, False)):
        got, _ = compare_with_restatement(p, gts, dts, [0], [1], metric, np.array([[0.7], [0.5]]), aos)
        assert got["precision"].max() > 0 and got["num_thresholds"].max() > 0


def test_empty_inputs():
    p = kitti_eval.pack([], [], DEV)
    for metric in range(3):
        assert p.overlaps(metric).numel() == 0
        ret = p.eval_class([0, 1], [0, 1, 2], metric, np.array([[0.7, 0.5]]), metric == 0, details=True)
        assert ret["precision"].shape == (2, 3, 1, 41) and not ret["precision"].any() and not ret["recall"].any()
        assert not ret["num_thresholds"].any().item() and not ret["num_valid_gt"].any().item()
    none = {k: np.zeros((0, w) if w else (0,)) for k, w in (("bbox", 4), ("location", 3), ("dimensions", 3), ("rotation_y", 0),
                                                              ("alpha", 0), ("score", 0), ("occluded", 0), ("truncated", 0))}
    none["name"] = np.zeros(0, dtype="<U8")
    result, ret = kitti_mirror.get_official_eval_result([none, none], [none, none], ["Car"])
    assert "bbox AP:0.0000, 0.0000, 0.0000" in result and "aos" not in result and all(v == 0 for v in ret.values())


def test_unsupported_is_refused():
    rng = np.random.default_rng(5)
    g, d = synthetic_frame(rng, 2, 4)
    big = {k: np.concatenate([v] * 257, 0) for k, v in d.items()}          # 1028 dets in one frame
    p = kitti_eval.pack([g], [big], DEV)
    with pytest.raises(_lib.LidarHipError, match="unsupported"):
        p.overlaps(0)
    with pytest.raises(_lib.LidarHipError, match="unsupported"):
        p.eval_class([0], [0], 0, np.array([[0.7]]))
    ok = kitti_eval.pack([g], [d], DEV)
    with pytest.raises(_lib.LidarHipError):
        ok.eval_class([0] * 9, [0], 0, np.full((1, 9), 0.7))
    with pytest.raises(_lib.LidarHipError):
        ok.eval_class([6], [0], 0, np.array([[0.7]]))
    with pytest.raises(_lib.LidarHipError):
        ok.eval_class([0], [0], 0, np.full((17, 1), 0.7))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (f) unchanged behaviour
@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
def test_rotate_iou_eval_bits_unchanged(criterion):
    """lidar_rotate_iou_eval after its geometry moved into csrc/eval_iou_dev.h: the bits recorded before the move, on the inputs
    of tests/test_gpu_roi_pool.py::test_kitti_eval_rotate_iou_matches_oracle"""
    z, tag = ke.fixture(), f"c{criterion + 1}"
    got = rotate_iou_gpu_eval(z[f"riou_boxes_{tag}"], z[f"riou_query_{tag}"], criterion)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), z[f"riou_out_{tag}"].view(np.uint32))
