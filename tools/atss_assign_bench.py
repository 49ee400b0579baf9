"""Times the ATSS anchor target assignment call (lidardetection_amd/atss_assign.py, csrc/atss_assign.hip: three
kernels) on synthetic gts over real anchor grids:

  kitti   PointPillar-KITTI training: bs 16, 3 sets x 107 136 anchors (248 x 216 x 2), TOPK 9, M 40 (about half the rows filled)
  nus     a multihead NuScenes shape: bs 4, 10 sets x 32 768 anchors (128 x 128 x 2, permuted), TOPK 9, M 60, code size 10

GPU time per call from device events around the whole window, host enqueue time per call, and the algorithmic output bytes (labels
+ targets + weights, all of which the call writes) over the GPU time as a fraction of the 8.0 TB/s HBM peak.  One JSON line.

Usage: python tools/atss_assign_bench.py [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd import atss_assign  # noqa: E402
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator  # noqa: E402

from _measure import event_and_enqueue_ms  # noqa: E402

HBM_PEAK = 8.0e12
KITTI_SIZES = [([3.9, 1.6, 1.56], -1.78), ([0.8, 0.6, 1.73], -0.6), ([1.76, 0.6, 1.73], -0.6)]
NUS_SIZES = [[4.63, 1.97, 1.74], [6.93, 2.51, 2.84], [6.37, 2.85, 3.19], [10.5, 2.94, 3.47], [12.29, 2.90, 3.87],
             [0.50, 2.53, 0.98], [2.11, 0.77, 1.47], [1.70, 0.60, 1.28], [0.73, 0.67, 1.77], [0.41, 0.41, 1.07]]


def shape(name, dev):
    r = np.random.default_rng(0)
    if name == "kitti":
        pc_range, grid, B, M, cols, multihead = [0, -39.68, -3, 69.12, 39.68, 1], [216, 248], 16, 40, 8, False
        sizes = KITTI_SIZES
    else:
        pc_range, grid, B, M, cols, multihead = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], [128, 128], 4, 60, 10, True
        sizes = [(s, -1.0) for s in NUS_SIZES]
    cfg = [dict(class_name=str(i), anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[h], align_center=False,
                feature_map_stride=1) for i, (s, h) in enumerate(sizes)]
    sets, _ = AnchorGenerator(pc_range, cfg).generate_anchors([grid] * len(cfg), device="cpu")
    if multihead:
        sets = [torch.nn.functional.pad(a, (0, 2)).permute(3, 4, 0, 1, 2, 5) for a in sets]
    flat = [a.contiguous().view(-1, a.shape[-1]).to(dev) for a in sets]
    gt = np.zeros((B, M, cols), np.float32)
    for b in range(B):
        for j in range(int(r.integers(M // 4, 3 * M // 4))):
            c = int(r.integers(0, len(sizes)))
            gt[b, j, :7] = [r.uniform(pc_range[0], pc_range[3]), r.uniform(pc_range[1], pc_range[4]), r.uniform(-1.5, 0),
                            *(np.array(sizes[c][0]) * r.uniform(0.8, 1.2, 3)), r.uniform(-np.pi, np.pi)]
            gt[b, j, -1] = c + 1
    code = 10 if multihead else 7
    return flat, torch.from_numpy(gt).to(dev), code, multihead


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("atss_assign_bench needs the GPU: a CPU run measures nothing")
    out = {}
    for name in ("kitti", "nus"):
        flat, gt, code, sincos = shape(name, "cuda:0")
        fn = lambda: atss_assign.assign(flat, gt, 9, code, sincos=sincos)  # noqa: E731
        for _ in range(args.warmup):
            labels, _, _ = fn()
        gpu_ms, host_ms = event_and_enqueue_ms(fn, args.steps)
        n = sum(a.shape[0] for a in flat)
        nbytes = gt.shape[0] * n * (4 + 4 * code + 4)
        out[name] = dict(batch=int(gt.shape[0]), sets=len(flat), anchors=n, max_gt=int(gt.shape[1]), topk=9,
                         positives=int((labels > 0).sum()), gpu_ms=round(gpu_ms, 4), host_ms=round(host_ms, 4),
                         output_mb=round(nbytes / 1e6, 1), output_gbps=round(nbytes / gpu_ms / 1e6, 1),
                         hbm_fraction=round(nbytes / (gpu_ms * 1e-3) / HBM_PEAK, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
