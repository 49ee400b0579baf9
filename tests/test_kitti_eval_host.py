"""KITTI AP evaluation, host side (lidardetection_amd/kitti_eval.py, csrc/kitti_eval.hip's pure-host entry points): the numpy
restatement of tests/_kitti_eval_np.py reproduces what the reference's own eval.py computed (tests/golden/kitti_eval_ref.npz, written
by tests/golden/make_kitti_eval_golden.py) from the overlaps the reference saw: thresholds and tp / fp / fn exactly, precision and
recall to 1e-12, AOS to 1e-9 (fp64 sums of at most a few thousand terms in [0, 1]).  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _kitti_eval_np as ke
from lidardetection_amd import _lib, kitti_eval

SETS = ("main", "noaos")


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", SETS)
def test_restatement_reproduces_reference(name, metric):
    s, got = ke.load_set(name), ke.restated(name, metric)
    n = 0
    for m in range(len(s["classes"])):
        for l in range(3):
            for k in range(2):
                thr, pr = s["thresholds"][metric][n], s["pr"][metric][n]
                assert got["thresholds"][m][l][k] == thr.tolist()
                assert np.array_equal(got["counts"][m, l, k, :len(thr)], pr[:, :3].astype(np.int64)) and np.array_equal(pr[:, :3], pr[:, :3].astype(np.int64))
                assert not got["counts"][m, l, k, len(thr):].any()
                n += 1
    assert np.abs(got["precision"] - s["precision"][metric]).max() <= 1e-12
    assert np.abs(got["recall"] - s["recall"][metric]).max() <= 1e-12
    assert np.abs(got["orientation"] - s["orientation"][metric]).max() <= 1e-9
    assert s["precision"][metric].max() > 0.5
    if metric == 0:
        assert (s["orientation"][0].max() > 0.3) == s["compute_aos"]


def test_restated_image_overlap_matches_recorded():
    s = ke.load_set("main")
    for g, d, ov in zip(s["gt_annos"], s["dt_annos"], s["overlaps"][0]):
        assert np.abs(ke.image_overlap(d["bbox"], g["bbox"]) - ov).max(initial=0) <= 1e-12


def test_map_rules_give_the_recorded_result():
    for name in SETS:
        s = ke.load_set(name)
        for j, cls in enumerate(s["classes"]):
            for key, metric in (("image", 0), ("bev", 1), ("3d", 2)):
                for level, word in enumerate(("easy", "moderate", "hard")):
                    want = s["ret_dict"][f"{ke.DISPLAY[cls]}_{key}/{word}_R40"]
                    assert abs(ke.map_r40(s["precision"][metric])[j, level, 0] - want) <= 1e-9
        line = f"bbox AP:{', '.join(f'{v:.4f}' for v in ke.map_r11(s['precision'][0])[0, :, 0])}\n"
        assert s["result"].split("\n", 1)[1].startswith(line)
        assert ("aos" in s["result"]) == s["compute_aos"]


def _flags(s, f, cls, diff):
    return ke.flags(s["gt_annos"][f], s["dt_annos"][f], cls, diff)


def test_fixture_holds_the_listed_cases():
    s = ke.load_set("main")
    gts, dts, ov = s["gt_annos"], s["dt_annos"], s["overlaps"]
    ng, nd = [len(a["name"]) for a in gts], [len(a["name"]) for a in dts]
    assert len(gts) == 24 and any(g == 0 < d for g, d in zip(ng, nd)) and any(d == 0 < g for g, d in zip(ng, nd))
    assert any(g == 0 == d for g, d in zip(ng, nd))
    # DontCare regions absorb dets that would be false positives (metric 0)
    f = next(i for i, a in enumerate(gts) if (a["name"] == "DontCare").any())
    _, gf, df = _flags(s, f, 0, 1)
    dc = ke.image_overlap(dts[f]["bbox"], gts[f]["bbox"][gts[f]["name"] == "DontCare"], 0)
    score = dts[f]["score"]
    assert ke.match(ov[0][f], gf, df, score, 0.7, 0.0, dc)[1] == 0 and ke.match(ov[0][f], gf, df, score, 0.7, 0.0, None)[1] == 2
    # a Van under a Car det, a Person_sitting under a Pedestrian det, a det of another class over a Car, an unknown class
    f = next(i for i, a in enumerate(gts) if (a["name"] == "Van").any())
    for cls, row, mo in ((0, 0, 0.7), (1, 1, 0.5)):
        _, gf, df = _flags(s, f, cls, 1)
        assert gf[row] == 1 and df[row] == 0 and all(ov[m][f][row, row] > mo for m in range(3))
    assert dts[f]["name"][2] == "Cyclist" and gts[f]["name"][2] == "Car" and ov[1][f][2, 2] > 0.7
    assert (gts[f]["name"] == "Tram").any() and (dts[f]["name"] == "tram").any() and (gts[f]["name"] == "Truck").any()
    # occlusion, truncation, height: ignored at easy, valid at hard
    f = next(i for i, a in enumerate(gts) if (a["truncated"] > 0.3).any())
    assert [_flags(s, f, 0, d)[1].tolist() for d in range(3)] == [[1, 1, 1], [0, 1, 0], [0, 0, 0]]
    assert gts[f]["occluded"][0] == 1 and gts[f]["truncated"][1] == 0.4 and 25 < gts[f]["bbox"][2, 3] - gts[f]["bbox"][2, 1] <= 40
    # too-small dets: the only match of gt 0 (third branch); under gt 1 the ignored det sits at the lower row
    f = next(i for i, a in enumerate(dts) if len(a["name"]) == 3 and (a["bbox"][:2, 3] - a["bbox"][:2, 1] < 25).all())
    _, gf, df = _flags(s, f, 1, 1)
    assert gf.tolist() == [0, 0] and df.tolist() == [1, 1, 0]
    for m, mo in ((0, 0.5), (1, 0.5), (2, 0.5)):
        o = ov[m][f]
        assert o[0, 0] > mo and o[1, 1] > mo and o[2, 1] > mo and o[1, 0] == 0 and o[2, 0] == 0
        assert ke.match(o, gf, df, dts[f]["score"], mo, 0.0)[:3] == (1, 0, 0)
    # the higher score has the lower overlap; identical duplicates
    f = next(i for i, a in enumerate(dts) if len(a["score"]) == 5 and a["score"][2] == a["score"][3])
    _, gf, df = _flags(s, f, 0, 0)
    sc = dts[f]["score"]
    for m in range(3):
        o = ov[m][f]
        assert sc[0] > sc[1] and o[1, 0] > o[0, 0] + 1e-3 > 0.7 and o[2, 1] == o[3, 1] > 0.7
        assert ke.match(o, gf, df, sc, 0.7)[:2] == [(0, sc[0]), (1, sc[2])]
        assert ke.match(o, gf, df, sc, 0.7, 0.0)[:3] == (3, 2, 0)
        assert ke.match(o, gf, df, sc, 0.7, 0.56)[:3] == (2, 1, 1)       # det 1 (score 0.55) is below the threshold: det 0 takes gt 0
    # no valid Cyclist at easy; more than 41 matched Car scores
    for metric in range(3):
        r = ke.restated("main", metric)
        assert r["num_valid_gt"][2, 0] == 0 and r["thresholds"][2][0] == [[], []] and not s["precision"][metric][2, 0].any()
        n_matched = sum(len(e) for e in r["matched"][0][2][1])
        assert n_matched > 41 and len(r["thresholds"][0][2][1]) < n_matched
    # margins: every overlap is exactly 0 or more than 1e-3 from every min_overlap in use
    for name in SETS:
        for metric in range(3):
            flat = np.concatenate([b.reshape(-1) for b in ke.load_set(name)["overlaps"][metric]])
            assert all(((np.abs(flat - t) > 1e-3) | (flat == 0)).all() for t in (0.7, 0.5, 0.25))
    assert ke.load_set("noaos")["dt_annos"][0]["alpha"][0] == -10 and not ke.load_set("noaos")["compute_aos"]


def test_packer_round_trip_and_names():
    s = ke.load_set("main")
    p = kitti_eval.pack(s["gt_annos"], s["dt_annos"], device="cpu")
    assert p.frames == 24 and p.total_gt == sum(len(a["name"]) for a in s["gt_annos"]) and p.gt.dtype == torch.float64
    assert p.gt.shape == (p.total_gt, kitti_eval.GT_COLS) and p.dt.shape == (p.total_dt, kitti_eval.DT_COLS)
    assert p.gt_off.dtype == torch.int32 and p.ov_off.dtype == torch.int64
    assert p.ov_off_host[-1] == sum(len(g["name"]) * len(d["name"]) for g, d in zip(s["gt_annos"], s["dt_annos"]))
    gts, dts = p.annos()
    for back, orig, keys in ((gts, s["gt_annos"], ke.GT_KEYS), (dts, s["dt_annos"], ke.DT_KEYS)):
        for a, b in zip(back, orig):
            assert all(np.array_equal(a[k], b[k]) for k in keys)
            for x, y in zip(a["name"], b["name"]):
                assert x == (y.lower() if y.lower() in ke.CLASSES else ("DontCare" if y == "DontCare" else "other"))
    ids = kitti_eval.class_ids(["Car", "CAR", "car", "Person_Sitting", "DontCare", "dontcare", "Tram", "truck", "Cyclist", "VAN"])
    assert ids.tolist() == [0, 0, 0, 4, 6, 7, 7, 5, 2, 3] and ids.dtype == np.int32
    with pytest.raises(_lib.LidarHipError):
        kitti_eval.pack(s["gt_annos"], s["dt_annos"][:-1], device="cpu")
    with pytest.raises(_lib.LidarHipError, match="CUDA"):           # no CPU path: the kernels refuse host tensors
        p.overlaps(0)
    with pytest.raises(_lib.LidarHipError, match="metric"):
        p.overlaps(3)


def test_supported_ranges():
    ok = kitti_eval.supported
    assert ok(0, 0, 0, 0, 0) and ok(3769, 30000, 45000, 256, 1024, 8, 3, 16) and ok(1 << 20, 1 << 20, 1 << 22, 1024, 1024, 8, 3, 16)
    assert not ok((1 << 20) + 1, 0, 0, 0, 0) and not ok(1, (1 << 20) + 1, 0, 1, 1) and not ok(1, 0, (1 << 22) + 1, 1, 1)
    assert not ok(1, 10, 10, 1025, 1) and not ok(1, 10, 10, 1, 1025) and not ok(-1, 0, 0, 0, 0) and not ok(1, -1, 0, 0, 0)
    assert not ok(1, 1, 1, 1, 1, 9) and not ok(1, 1, 1, 1, 1, 0) and not ok(1, 1, 1, 1, 1, 1, 4) and not ok(1, 1, 1, 1, 1, 1, 0)
    assert not ok(1, 1, 1, 1, 1, 1, 1, 17) and not ok(1, 1, 1, 1, 1, 1, 1, 0)


def test_workspace_bytes_monotone():
    base = dict(frames=24, total_gt=150, total_dt=160, max_gt=9, max_dt=9, num_class=3, num_diff=3, num_overlap=2)
    b0 = kitti_eval.workspace_bytes(**base)
    assert b0 >= 18 * 24 * 41 * 20 + 9 * 310
    for key, values in [("frames", (0, 1, 24, 25, 4000)), ("total_gt", (0, 1, 150, 256, 257, 40000)), ("total_dt", (0, 150, 160, 50000)),
                        ("max_gt", (0, 9, 1024)), ("max_dt", (0, 9, 1024)), ("num_class", range(1, 9)), ("num_diff", (1, 2, 3)),
                        ("num_overlap", range(1, 17))]:
        sizes = [kitti_eval.workspace_bytes(**{**base, key: v}) for v in values]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, key
    assert kitti_eval.workspace_bytes(**{**base, "max_dt": 1025}) == 0 and kitti_eval.workspace_bytes(**{**base, "num_class": 9}) == 0


def test_c_abi_refusals():
    """every refusal comes before any launch: the pointers below are dummies that are never read"""
    L = _lib.lib()
    p = C.c_void_p(256)
    ARG, UNSUPPORTED, WORKSPACE = -1, -4, -3

    def overlaps(metric=0, gt=p, dt=p, go=p, do=p, oo=p, frames=2, tg=5, td=6, ot=15, mg=3, md=3, out=p):
        return L.lidar_kitti_eval_overlaps(metric, -1, gt, dt, go, do, oo, frames, tg, td, ot, mg, md, out, None)

    assert overlaps(metric=3) == ARG and overlaps(metric=-1) == ARG
    assert overlaps(frames=-1) == ARG and overlaps(tg=-1) == ARG and overlaps(td=-1) == ARG and overlaps(ot=-1) == ARG
    assert overlaps(mg=-1) == ARG and overlaps(md=-1) == ARG
    for name in ("gt", "dt", "go", "do", "oo", "out"):
        assert overlaps(**{name: None}) == ARG, name
    assert overlaps(mg=1025) == UNSUPPORTED and overlaps(md=1025) == UNSUPPORTED and overlaps(frames=(1 << 20) + 1) == UNSUPPORTED
    assert overlaps(tg=(1 << 20) + 1) == UNSUPPORTED and overlaps(td=(1 << 22) + 1) == UNSUPPORTED
    assert overlaps(frames=0) == 0 and overlaps(ot=0, gt=None, dt=None, out=None) == 0          # nothing to do: no launch

    classes, diffs, mo = _lib.host_i32([0, 1]), _lib.host_i32([0, 2]), (C.c_double * 4)(0.7, 0.5, 0.5, 0.25)

    def eval_class(metric=1, gt=p, dt=p, gc=p, dc_=p, go=p, do=p, oo=p, ov=p, dcov=None, frames=2, tg=5, td=6, ot=15, mg=3, md=3,
                   classes=classes, nc=2, diffs=diffs, nd=2, mo=mo, nk=2, matched=p, nv=p, thr=p, nthr=p, counts=p, curves=p, ws=p,
                   ws_bytes=1 << 30):
        return L.lidar_kitti_eval_class(metric, gt, dt, gc, dc_, go, do, oo, ov, dcov, frames, tg, td, ot, mg, md, classes, nc, diffs,
                                        nd, mo, nk, 0, matched, nv, thr, nthr, counts, curves, ws, ws_bytes, None)

    assert eval_class(metric=3) == ARG and eval_class(metric=-1) == ARG
    for name in ("frames", "tg", "td", "ot", "mg", "md", "nc", "nd", "nk"):
        assert eval_class(**{name: -1}) == ARG, name
    for name in ("gt", "dt", "gc", "dc_", "go", "do", "oo", "ov", "classes", "diffs", "mo", "matched", "nv", "thr", "nthr", "counts", "curves"):
        assert eval_class(**{name: None}) == ARG, name
    assert eval_class(metric=0) == ARG                                   # metric 0 needs the dt x DontCare overlaps
    assert eval_class(classes=_lib.host_i32([0, 6])) == ARG and eval_class(diffs=_lib.host_i32([0, 3])) == ARG
    assert eval_class(mg=1025) == UNSUPPORTED and eval_class(md=1025) == UNSUPPORTED and eval_class(tg=(1 << 20) + 1) == UNSUPPORTED
    assert eval_class(nc=9, classes=_lib.host_i32([0] * 9)) == UNSUPPORTED and eval_class(nd=4, diffs=_lib.host_i32([0] * 4)) == UNSUPPORTED
    assert eval_class(nk=17) == UNSUPPORTED and eval_class(nc=0) == UNSUPPORTED
    need = L.lidar_kitti_eval_workspace_bytes(2, 5, 6, 3, 3, 2, 2, 2)
    assert need > 0 and eval_class(ws_bytes=need - 1) == WORKSPACE and eval_class(ws=None) == WORKSPACE
