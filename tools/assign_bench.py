"""Times anchor target assignment: the HIP assigner (lidardetection_amd AxisAlignedTargetAssigner) against the torch restatement
of the reference algorithm in tests/_anchor_assign_torch.py (per frame and anchor class, full IoU matrix, argmax on the host),
at PointPillar-KITTI bs 16 (216 x 248 x 6 = 321 408 anchors per frame) and SECOND-MultiHead-NuScenes bs 4 (10 classes x 128 x 128
x 2 = 327 680 anchors, sincos coder, 9-column gts).  Device events per call after warm-up (_measure.event_ms); prints one JSON line.

  python tools/assign_bench.py [--iters 50] [--ref-iters 3] [--rocprof OUTDIR]

--rocprof OUTDIR: afterwards runs this script again (HIP assigner only) in a child process under
`rocprofv3 --kernel-trace --stats -d OUTDIR`, so the kernel statistics come from a run of their own.
HBM floor: bytes written (labels 4 + targets 4 * code_size + weights 4 per anchor and frame) at 8 TB/s.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))    # the workload builders and restatements the tests use

from lidardetection_amd.pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator  # noqa: E402
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import \
    AxisAlignedTargetAssigner  # noqa: E402

import _anchor_assign_torch as T  # noqa: E402
from _measure import event_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def workload(name, dev, seed=3):
    if name == "pointpillar_kitti_bs16":
        meta, anchors, gt = T.kitti_production(dev, batch=16, seed=seed)
        return meta, anchors, gt, T.Coder(7, False), 7, False
    meta = T.load_case("nus")[0]
    meta["anchor_generator_config"] = [dict(c, feature_map_stride=8) for c in meta["anchor_generator_config"]]
    gen = AnchorGenerator(meta["pc_range"], meta["anchor_generator_config"])
    anchors, _ = gen.generate_anchors([[128, 128]] * 10, device=dev)
    anchors = [torch.cat((a, a.new_zeros([*a.shape[:-1], 3])), dim=-1) for a in anchors]     # padded to code_size 10
    r = np.random.default_rng(seed)
    B, M = 4, 60
    gt = np.zeros((B, M, 10), np.float32)
    sizes = [c["anchor_sizes"][0] for c in meta["anchor_generator_config"]]
    for b in range(B):
        for j in range(int(r.integers(20, M + 1))):
            c = int(r.integers(1, 11))
            gt[b, j] = [r.uniform(-50, 50), r.uniform(-50, 50), r.uniform(-2, 1), *(np.array(sizes[c - 1]) * r.uniform(0.8, 1.2, 3)),
                        r.uniform(-np.pi, np.pi), *r.normal(0, 3, 2), c]
    return meta, anchors, torch.from_numpy(gt).to(dev), T.Coder(9, True), 10, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ref-iters", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--rocprof", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("assign_bench: no GPU")
    dev = torch.device("cuda:0")
    result = {"tool": "assign_bench", "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in ["pointpillar_kitti_bs16", "second_multihead_nuscenes_bs4"]:
        meta, anchors, gt, coder, code, sincos = workload(name, dev)
        cfg = T.model_cfg(meta)
        a = AxisAlignedTargetAssigner(cfg, meta["class_names"], coder)
        hip = lambda: a.assign_targets(anchors, gt)   # noqa: E731
        med, lo, hi = event_ms(hip, args.iters, 5)
        B, N = hip()["box_cls_labels"].shape
        written = B * N * (4 + 4 * code + 4)
        w = {"batch": B, "anchors_per_frame": N, "hip_ms_median": round(med, 4), "hip_ms_min": round(lo, 4),
             "hip_ms_max": round(hi, 4), "bytes_written": written, "hbm_floor_ms": round(written / HBM_BYTES_PER_S * 1e3, 4)}
        if not args.hip_only:
            ref = lambda: T.restated_assign(cfg, meta["class_names"], code, sincos, anchors, gt)   # noqa: E731
            rmed, rlo, rhi = event_ms(ref, args.ref_iters, 1)
            w.update({"restated_ms_median": round(rmed, 3), "restated_ms_min": round(rlo, 3), "speedup": round(rmed / med, 1)})
            got, exp = hip(), ref()
            T.assert_targets_match(got, exp, sincos)
            w["matches_restatement"] = True
        result["workloads"][name] = w
    print(json.dumps(result), flush=True)
    if args.rocprof:
        # `timeout -k 10` bounds the whole process group, the profiled Python child included
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", args.rocprof, "-o", "assign", "--",
               sys.executable, os.path.abspath(__file__), "--hip-only", "--iters", "20"]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"assign_bench: rocprofv3 pass exited with {rc}")


if __name__ == "__main__":
    main()
