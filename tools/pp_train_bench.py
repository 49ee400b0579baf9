"""Times PointPillar-KITTI training at bs 16 with the fused train-mode PillarVFE + differentiable scatter (csrc/pfn_train.hip)
against the mirror's torch formulation of the same layer (pcdet/models/backbones_3d/vfe/encoders.py PFNLayer, index-assign
scatter), and reports the peak device memory of each:

  pfn_scatter  PFN + scatter forward + backward (gradients of the linear weight and the norm's weight / bias) on a fixed
               channels-last canvas gradient;
  full_step    PointPillarKITTI.train_loss + backward, against the same step on the torch PFN (float32) and scatter (the stock
               step of tests/_pp_train_torch.py).

Inputs: 16 synthetic KITTI-like clouds (8 uniform, 8 ring) through BatchVoxelizer at 16 000 voxels per frame.  Device events per call after
warm-up (_measure.event_ms), the median of --iters; peak memory from torch.cuda.max_memory_allocated above what was allocated before the call.
Prints one JSON line.

  python tools/pp_train_bench.py [--iters 20] [--rocprof OUTDIR]

--rocprof OUTDIR: afterwards runs this script again (fused paths only) in a child process under
`rocprofv3 --kernel-trace --stats --output-format csv -d OUTDIR`, so the kernel statistics come from a run of their own.
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

from lidardetection_amd import pillar_ops, synth  # noqa: E402

import _pp_train_torch as T  # noqa: E402
from _measure import event_ms, peak_mb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--rocprof", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pp_train_bench: no GPU")
    dev = T.DEV
    B = 16
    vox, nv = T.bs16_voxels(B=B)
    total = vox["voxel_offsets"][B:B + 1]
    m = T.vfe()
    layer = m.pfn_layers[0]
    params = [layer.linear.weight, layer.norm.weight, layer.norm.bias]
    G = torch.randn(B, 64, 496, 432, device=dev).contiguous(memory_format=torch.channels_last)
    v_live, n_live, c_live = vox["voxels"][:nv], vox["voxel_num_points"][:nv], vox["voxel_coords"][:nv]

    def fused_pfn():
        out = pillar_ops.pillar_vfe_train(vox["voxels"], vox["voxel_num_points"], vox["voxel_coords"], *params,
                                          layer.norm.running_mean, layer.norm.running_var, synth.PP_VOXEL, synth.PP_RANGE,
                                          num_batches_tracked=layer.norm.num_batches_tracked, num_voxels_dev=total)
        canvas = pillar_ops.pillar_scatter_train(out, vox["voxel_coords"], B, 432, 496, num_voxels_dev=total, channels_last=True)
        torch.autograd.grad((canvas * G).sum(), params)

    def torch_pfn():      # the mirror's torch formulation (encoders.py PillarVFE._decorate + PFNLayer, bev_maps.py index-assign)
        feats = m._decorate(v_live, n_live, c_live)
        feats = layer(feats).squeeze(1)
        flat = feats.new_zeros((B, 64, 496 * 432))
        c = c_live.long()
        flat[c[:, 0], :, c[:, 2] * 432 + c[:, 3]] = feats
        canvas = flat.view(B, 64, 496, 432).contiguous(memory_format=torch.channels_last)
        torch.autograd.grad((canvas * G).sum(), params)

    result = {"tool": "pp_train_bench", "device": torch.cuda.get_device_name(0), "batch": B, "pillars": nv,
              "padded_rows": int(vox["voxels"].shape[0])}
    med, mn, _ = event_ms(fused_pfn, args.iters, 3)
    w = {"fused_ms_median": round(med, 4), "fused_ms_min": round(mn, 4), "fused_peak_mb": peak_mb(fused_pfn)}
    if not args.fused_only:
        med_t, mn_t, _ = event_ms(torch_pfn, args.iters, 3)
        w.update({"torch_ms_median": round(med_t, 3), "torch_ms_min": round(mn_t, 3), "torch_peak_mb": peak_mb(torch_pfn),
                  "speedup": round(med_t / med, 1)})
    result["pfn_scatter"] = w

    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = T.pp_inputs(B, 5)
    torch.manual_seed(4)
    pp = PointPillarKITTI(batch_size=B, device=dev).train()
    pparams = [p for p in pp.parameters() if p.requires_grad]
    fused_step = lambda: torch.autograd.grad(sum(pp.train_loss(pts, offs, gt)), pparams)                 # noqa: E731
    stock_step = lambda: torch.autograd.grad(sum(T.stock_loss(pp, pts, offs, gt, torch.float32)), pparams)            # noqa: E731
    med, mn, _ = event_ms(fused_step, max(args.iters // 2, 3), 2)
    w = {"fused_ms_median": round(med, 3), "fused_ms_min": round(mn, 3), "fused_peak_mb": peak_mb(fused_step)}
    if not args.fused_only:
        med_t, mn_t, _ = event_ms(stock_step, max(args.iters // 2, 3), 2)
        w.update({"torch_ms_median": round(med_t, 3), "torch_ms_min": round(mn_t, 3), "torch_peak_mb": peak_mb(stock_step),
                  "speedup": round(med_t / med, 2)})
    result["full_step"] = w
    print(json.dumps(result), flush=True)
    if args.rocprof:
        # `timeout -k 10` bounds the whole process group, the profiled Python child included
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.rocprof,
               "-o", "pp_train", "--",
               sys.executable, os.path.abspath(__file__), "--fused-only", "--iters", "5"]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"pp_train_bench: rocprofv3 pass exited with {rc}")


if __name__ == "__main__":
    main()
