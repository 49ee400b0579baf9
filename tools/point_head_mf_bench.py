"""Times the multi-frame point head at the load of tools/cfgs/livox_models/pv_rcnn_multiframe.yaml at bs 8: N = 8 x 4086 keypoints,
M = 64 gt rows, S = 3 stacked sweeps.  Two columns, on the same tensors in the same process:

  fused     lidardetection_amd/point_head_mf.py: targets of all S frames (one launch) + loss forward + backward
  s_calls   S calls of the single-frame point_head.assign_point_targets on gt boxes with the centre and heading of frame s
            substituted, the labels stacked, and the mirror's torch formulation of the multi-frame loss with its autograd backward

Reports per column: wall time per call (device events, median and minimum after warm-up), host time to enqueue, the number of device
kernels and device-to-host copies (torch.profiler).  Prints one JSON line.

  python tools/point_head_mf_bench.py [--iters 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from point_head_bench import scene  # noqa: E402
from _measure import enqueue_ms, event_ms, kernel_count  # noqa: E402
from lidardetection_amd import point_head, point_head_mf  # noqa: E402
from lidardetection_amd.pcdet.models.dense_heads import PointHeadSimpleMultiFrame  # noqa: E402
from lidardetection_amd.pcdet.utils.cfg import AttrDict  # noqa: E402

B, K, M, S = 8, 4086, 64, 3
CFG = dict(CLS_FC=[], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True, TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
           LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0)))


def to_cfg(d):
    return AttrDict({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("point_head_mf_bench: no GPU")
    dev = torch.device("cuda:0")
    pts, gt = scene(B, K, M - 8, 5)                              # M - 8 real rows and 8 rows of zero padding
    r = np.random.default_rng(6)
    real = (gt[..., 3] > 0)[..., None]
    step = np.cumsum(r.normal(0, 0.5, (B, M, S, 3)) * np.float32([1, 1, 0.05]), axis=2)
    turn = np.cumsum(r.normal(0, 0.1, (B, M, S)), axis=2)
    step[:, :, 0], turn[:, :, 0] = 0, 0
    loc = np.where(real[..., None], gt[:, :, None, 0:3] + step, 0).astype(np.float32)
    rot = np.where(real, gt[:, :, None, 6] + turn, 0).astype(np.float32)
    pts, gt, loc, rot = (torch.from_numpy(a).to(dev) for a in (pts, gt, loc, rot))
    n = pts.shape[0]
    spec = point_head_mf.spec_from_cfg(CFG, 1)
    head = PointHeadSimpleMultiFrame(num_class=1, input_channels=4, model_cfg=to_cfg(CFG), stack_frame_size=S)
    x = torch.randn((n, S), device=dev).requires_grad_(True)

    def fused():
        x.grad = None
        t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
        cls, _ = point_head_mf.point_head_loss_mf(x, t, spec, S)
        cls.backward()

    def s_calls():
        x.grad = None
        cols = []
        for s in range(S):
            sub = gt.clone()
            sub[..., 0:3], sub[..., 6] = loc[:, :, s], rot[:, :, s]
            cols.append(point_head.assign_point_targets(pts, sub, spec)["point_cls_labels"])
        cls, _ = head._torch_terms_mf(x, torch.stack(cols, dim=-1))
        cls.backward()

    t = point_head_mf.assign_point_targets_mf(pts, gt, loc, rot, spec)
    lab = t["point_cls_labels_stacked"]
    result = {"tool": "point_head_mf_bench", "device": torch.cuda.get_device_name(0), "batch": B, "points": n, "gt_rows": M,
              "stack_frame_size": S, "positives": int((lab > 0).sum()), "ignored": int((lab < 0).sum())}
    for col, fn in (("fused", fused), ("s_calls", s_calls)):
        med, lo, _ = event_ms(fn, args.iters, 10)
        k = kernel_count(fn)
        result[col] = {"wall_ms_median": round(med, 4), "wall_ms_min": round(lo, 4), "enqueue_ms": round(enqueue_ms(fn, args.iters), 4),
                       "device_kernels": k["kernels"], "device_to_host_copies": k["d2h_copies"]}
        if col == "fused":
            result[col]["kernel_names"] = k["names"]
    result["speedup_wall"] = round(result["s_calls"]["wall_ms_median"] / result["fused"]["wall_ms_median"], 2)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
