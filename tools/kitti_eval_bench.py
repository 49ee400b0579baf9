"""Times the KITTI AP evaluation on the device (lidardetection_amd/kitti_eval.py, csrc/kitti_eval.hip, the eval.py mirror) on a
synthetic set of the KITTI val size: 3769 frames, about 8 gt and 12 dt per frame, classes Car / Pedestrian / Cyclist.

Reported: wall time of get_official_eval_result end to end (packing on the host, three metrics, the result string; ends in the
curves' device read), and of its parts: packing, the overlaps of each metric, eval_class of each metric (host clock around work
that ends in a device synchronise).  There is nothing to compare it against: the reference's numba code cannot run here, and its
plain-Python form is not its real speed.  One JSON line.

Usage: python tools/kitti_eval_bench.py [--frames 3769] [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd import kitti_eval  # noqa: E402
from lidardetection_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_mirror  # noqa: E402

from _measure import host_ms  # noqa: E402

SIZES = {"Car": (3.9, 1.5, 1.6), "Pedestrian": (0.8, 1.75, 0.6), "Cyclist": (1.76, 1.7, 0.6), "Van": (5.0, 2.2, 2.0)}
NAMES = ["Car", "Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Van", "DontCare"]


def synthetic_set(frames, seed=0):
    r = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(frames):
        n = int(r.integers(4, 13))
        names = r.choice(NAMES, n)
        dims = np.array([SIZES.get(str(c), (1.0, 1.0, 1.0)) for c in names]) * r.uniform(0.9, 1.1, (n, 3))
        loc = np.stack([r.uniform(-30, 30, n), np.full(n, 1.6), r.uniform(8, 70, n)], 1)
        hpx = 720.0 * dims[:, 1] / loc[:, 2]
        u, wpx = 610.0 + 720.0 * loc[:, 0] / loc[:, 2], 500.0 * dims[:, 0] / loc[:, 2]
        bottom = 175.0 + 720.0 * 1.6 / loc[:, 2]
        gt = dict(name=names.astype("<U16"), bbox=np.stack([u - wpx / 2, bottom - hpx, u + wpx / 2, bottom], 1), location=loc,
                  dimensions=dims, rotation_y=r.uniform(-np.pi, np.pi, n), alpha=r.uniform(-np.pi, np.pi, n),
                  occluded=r.integers(0, 3, n).astype(np.float64), truncated=r.choice([0.0, 0.0, 0.2, 0.6], n))
        real = np.nonzero(names != "DontCare")[0]
        pick = np.concatenate([real[r.random(len(real)) < 0.85], r.choice(real, int(r.integers(2, 8)))]) if len(real) else real
        m = len(pick)
        dt = dict(name=gt["name"][pick], bbox=gt["bbox"][pick] + r.normal(0, 2.0, (m, 4)),
                  location=loc[pick] + r.normal(0, 0.15, (m, 3)) * [1, 0.2, 1], dimensions=dims[pick] * r.uniform(0.95, 1.05, (m, 3)),
                  rotation_y=gt["rotation_y"][pick] + r.normal(0, 0.05, m), alpha=gt["alpha"][pick] + r.normal(0, 0.1, m),
                  score=r.uniform(0.05, 1.0, m))
        gts.append(gt)
        dts.append(dt)
    return gts, dts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kitti_eval_bench needs the GPU: a CPU run measures nothing")
    gts, dts = synthetic_set(args.frames)
    classes = ["Car", "Pedestrian", "Cyclist"]
    full = lambda: kitti_mirror.get_official_eval_result(gts, dts, classes)  # noqa: E731
    for _ in range(args.warmup):
        result, _ = full()
    out = dict(frames=args.frames, gt=sum(len(a["name"]) for a in gts), dt=sum(len(a["name"]) for a in dts),
               official_result_ms=round(host_ms(full, args.steps), 2),
               pack_ms=round(host_ms(lambda: kitti_eval.pack(gts, dts, "cuda:0"), args.steps), 2))
    table = kitti_mirror.MIN_OVERLAPS[:, :, [0, 1, 2]]
    for metric, key in enumerate(("bbox", "bev", "3d")):
        p = kitti_eval.pack(gts, dts, "cuda:0")
        t_ov = []
        for _ in range(args.steps):
            p._overlaps.clear()
            t_ov.append(host_ms(lambda: [p.overlaps(metric)] + ([p.overlaps(0, 0)] if metric == 0 else []), 1))
        out[f"{key}_overlaps_ms"] = round(float(np.mean(t_ov)), 3)
        out[f"{key}_eval_class_ms"] = round(host_ms(lambda: p.eval_class([0, 1, 2], [0, 1, 2], metric, table[:, metric, :], metric == 0),
                                                 args.steps), 3)
    out["first_lines"] = result.split("\n")[:4]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
