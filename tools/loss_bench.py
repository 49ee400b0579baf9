"""Times the fused anchor-head loss (lidardetection_amd/anchor_loss.py) against the torch restatement of the reference's get_loss in
tests/_anchor_loss_torch.py (fp32, autograd), forward alone and forward + backward, at PointPillar-KITTI bs 16 (321 408 anchors per
frame, 3 classes, code 7, 2 direction bins) and SECOND-MultiHead-NuScenes bs 4 (6 heads, 327 680 anchors, code 10, WeightedL1Loss,
no direction classifier).  Labels and targets come from the GPU assigner (the workloads of the same module).  Device
events per call after warm-up (_measure.event_ms); prints one JSON line.

  python tools/loss_bench.py [--iters 50] [--ref-iters 10] [--rocprof OUTDIR]

--rocprof OUTDIR: afterwards runs this script again (fused loss only) in a child process under
`rocprofv3 --kernel-trace --stats -d OUTDIR`, so the kernel statistics come from a run of their own.
HBM floor, from shapes at 8 TB/s: forward reads cls + box + dir logits, targets and the label of every anchor; backward reads the
same and writes the three gradients.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))    # the workload builders and restatements the tests use

from lidardetection_amd import anchor_loss  # noqa: E402

import _anchor_loss_torch as T  # noqa: E402
from _measure import event_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ref-iters", type=int, default=10)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--rocprof", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench: no GPU")
    result = {"tool": "loss_bench", "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in ["pointpillar_kitti_bs16", "second_multihead_nuscenes_bs4"]:
        if name.startswith("pointpillar"):
            _, head, t, cls, box, dirs, _ = T.pp_case(B=16, seed=0)
        else:
            _, head, t, cls, box, _ = T.nus_case(B=4, seed=1)
            dirs = []
        spec, anchors = head.loss_spec, head.loss_anchors()
        labels, targets = t['box_cls_labels'], t['box_reg_targets']
        B, N = labels.shape
        nh = len(cls)
        leaves = [x.clone().requires_grad_() for x in cls + box + dirs]
        pick = lambda xs: xs if nh > 1 else xs[0]   # noqa: E731

        def fused(backward):
            losses = anchor_loss.anchor_head_loss(pick(leaves[:nh]), pick(leaves[nh:2 * nh]),
                                                  pick(leaves[2 * nh:]) if dirs else None, labels, targets, anchors, spec)
            if backward:   # fresh gradients each call (no accumulation into .grad), as the restatement below
                torch.autograd.grad(list(losses), leaves)

        with torch.no_grad():
            fwd_med, fwd_min, _ = event_ms(lambda: fused(False), args.iters, 5)
        fb_med, fb_min, _ = event_ms(lambda: fused(True), args.iters, 5)
        code, bins = len(spec.code_weights), spec.num_dir_bins if dirs else 0
        cls_cols = sum(int(x.numel()) for x in cls) // (B * N)    # class logits per anchor (multihead: each head's own)
        read = B * N * 4 * (cls_cols + code + bins + code + 1)
        written = B * N * 4 * (cls_cols + code + bins)
        w = {"batch": B, "anchors_per_frame": N, "heads": nh, "positives": int((labels > 0).sum()),
             "fused_fwd_ms_median": round(fwd_med, 4), "fused_fwd_ms_min": round(fwd_min, 4),
             "fused_fwd_bwd_ms_median": round(fb_med, 4), "fused_fwd_bwd_ms_min": round(fb_min, 4),
             "floor_fwd_ms": round(read / HBM_BYTES_PER_S * 1e3, 4),
             "floor_fwd_bwd_ms": round((2 * read + written) / HBM_BYTES_PER_S * 1e3, 4)}
        if not args.fused_only:
            def restated():
                rl = [x.detach().requires_grad_() for x in leaves]
                widths = [x.shape[-1] if nh > 1 else spec.num_class for x in cls] + [code] * nh + [bins] * len(dirs)
                views = [x.reshape(B, -1, c) for x, c in zip(rl, widths)]
                losses = T.restated_loss(views[:nh], views[nh:2 * nh], views[2 * nh:], labels, targets, anchors, spec)
                torch.autograd.grad([x for x in losses if x.requires_grad], rl)
            r_med, r_min, _ = event_ms(restated, args.ref_iters, 2)
            w.update({"restated_fwd_bwd_ms_median": round(r_med, 3), "restated_fwd_bwd_ms_min": round(r_min, 3),
                      "speedup": round(r_med / fb_med, 1)})
        result["workloads"][name] = w
    print(json.dumps(result), flush=True)
    if args.rocprof:
        # `timeout -k 10` bounds the whole process group, the profiled Python child included
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", args.rocprof, "-o", "loss", "--",
               sys.executable, os.path.abspath(__file__), "--fused-only", "--iters", "20"]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"loss_bench: rocprofv3 pass exited with {rc}")


if __name__ == "__main__":
    main()
