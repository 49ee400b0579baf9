"""Times what the multi-frame poses cost the train-time augmentation (csrc/augment.hip) on the load of pv_rcnn_multiframe.yaml at batch 8:
8 frames of about 19 000 points with C = 5 features, S = 3 stacked sweeps, 15 candidates in each of 3 groups, road plane, sample
rotation, flip / rotation / scaling.  Two pairs, each from device events around single calls (median of --iters calls after a warm-up,
the whole measurement run twice):
  * lidar_augment_mf against lidar_augment of the same build on the same inputs: the price of the poses;
  * lidar_augment of this build against lidar_augment of another build of the library (--parent-so, e.g. the parent commit's), the two
    interleaved call by call: whether the shared kernel slowed the single-frame path.
One JSON line.  Usage: python tools/augment_mf_bench.py [--parent-so path/to/liblidar_hip.so] [--batch 8] [--frames 3] [--iters 200]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _augment_mf_np as amf  # noqa: E402
from augment_bench import make_batch  # noqa: E402
from lidardetection_amd import _lib  # noqa: E402


def bind_plain(path):
    """lidar_augment of another build of the library, which need not export what this build's header declares"""
    so = ctypes.CDLL(path)
    so.lidar_augment.restype, so.lidar_augment.argtypes = _lib.SIGNATURES["lidar_augment"]
    return so.lidar_augment


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-so", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_mf_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = "cuda:0"
    inp, cfg = make_batch(args.batch)
    r = np.random.default_rng(1)
    for k in ("points", "db_points"):                                   # C = 5
        inp[k] = np.concatenate([inp[k], r.uniform(0, 1, (len(inp[k]), 1)).astype(np.float32)], 1)
    inp = amf.add_poses(inp, args.frames)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)      # noqa: E731
    f32, i32 = np.float32, np.int32
    d = {k: up(inp[k], t) for k, t in (
        ("points", f32), ("point_offsets", i32), ("gt_boxes", f32), ("gt_counts", i32), ("db_points", f32), ("db_offsets", i32),
        ("db_boxes", f32), ("db_cls", i32), ("cand", i32), ("flip_x", i32), ("flip_y", i32), ("rot", f32), ("scale", f32),
        ("sample_rot", f32), ("plane", f32), ("locations", f32), ("rotations_y", f32), ("db_locations", f32), ("db_rotations_y", f32))}
    rot64 = inp["rot"].astype(np.float64)
    d["cs"] = up(np.stack([np.cos(rot64), np.sin(rot64)], 1), f32)
    B, G, P = inp["cand"].shape
    M, (n, C), F = inp["gt_boxes"].shape[1], inp["points"].shape, args.frames
    sizes = np.diff(inp["db_offsets"])
    bound = int(sizes[inp["cand"]].sum())
    cap = n + bound
    L, p = _lib.lib(), _lib.ptr

    def outputs():
        return dict(points=torch.zeros((cap, C), device=dev), point_offsets=torch.zeros(B + 1, dtype=torch.int32, device=dev),
                    gt_boxes=torch.zeros((B, M + G * P, 8), device=dev), gt_counts=torch.zeros(B, dtype=torch.int32, device=dev),
                    sample_valid=torch.zeros((B, G, P), dtype=torch.int32, device=dev), locations=torch.zeros((B, M + G * P, F, 3), device=dev),
                    rotations_y=torch.zeros((B, M + G * P, F), device=dev))

    o_mf, o_plain, o_parent = outputs(), outputs(), outputs()
    ws = torch.empty(int(L.lidar_augment_workspace_bytes(B, G, P, cap)), dtype=torch.uint8, device=dev)
    head = (p(d["points"]), p(d["point_offsets"]), n, C, p(d["gt_boxes"]), p(d["gt_counts"]), B, M, p(d["db_points"]), p(d["db_offsets"]),
            p(d["db_boxes"]), p(d["db_cls"]), len(sizes), int(inp["db_points"].shape[0]), p(d["cand"]), G, P, p(d["flip_x"]), p(d["flip_y"]),
            p(d["rot"]), p(d["cs"]), p(d["scale"]), p(d["sample_rot"]), p(d["plane"]), _lib.host_f32(cfg["remove_extra_width"]), None,
            _lib.host_f32(cfg["pc_range"]), 1, 1, bound, cap)

    def outs(o):
        return p(o["points"]), p(o["point_offsets"]), p(o["gt_boxes"]), p(o["gt_counts"]), p(o["sample_valid"])

    calls = {
        "mf": lambda: L.lidar_augment_mf(*head, p(d["locations"]), p(d["rotations_y"]), p(d["db_locations"]), p(d["db_rotations_y"]), F,
                                         *outs(o_mf), p(o_mf["locations"]), p(o_mf["rotations_y"]), p(ws), ws.numel(), _lib.stream()),
        "plain": lambda: L.lidar_augment(*head, *outs(o_plain), p(ws), ws.numel(), _lib.stream()),
    }
    if args.parent_so:
        parent = bind_plain(args.parent_so)
        calls["parent_plain"] = lambda: parent(*head, *outs(o_parent), p(ws), ws.numel(), _lib.stream())

    def measure():
        """median device time of every call, the calls interleaved so that drift meets all of them alike -> {name: ms}"""
        for _ in range(args.warmup):
            for fn in calls.values():
                assert fn() == 0
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        for _ in range(args.iters):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}

    runs = [measure(), measure()]
    shared = ("points", "point_offsets", "gt_boxes", "gt_counts", "sample_valid")
    assert all(torch.equal(o_mf[k], o_plain[k]) for k in shared), "the multi-frame call's shared outputs differ from the plain call's"
    if args.parent_so:
        assert all(torch.equal(o_parent[k], o_plain[k]) for k in shared), "the plain call's outputs differ from the other build's"
    res = dict(bench="augment_mf", batch=B, stack_frames=F, features=C, points_in=n, points_out=int(o_mf["point_offsets"][-1]),
               candidates=int(G * P), samples_valid=int(o_mf["sample_valid"].sum()), boxes_out=int(o_mf["gt_counts"].sum()),
               iters=args.iters, device=torch.cuda.get_device_name(0))
    for k in calls:
        res[f"{k}_ms_runs"] = [round(run[k], 4) for run in runs]
    res["poses_cost_us_runs"] = [round((run["mf"] - run["plain"]) * 1e3, 2) for run in runs]
    if args.parent_so:
        res["plain_minus_parent_us_runs"] = [round((run["plain"] - run["parent_plain"]) * 1e3, 2) for run in runs]
        res["plain_run_to_run_us"] = round(abs(runs[0]["plain"] - runs[1]["plain"]) * 1e3, 2)
        res["parent_run_to_run_us"] = round(abs(runs[0]["parent_plain"] - runs[1]["parent_plain"]) * 1e3, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
