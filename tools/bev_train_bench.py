"""Times the bs-16 PointPillar-KITTI training step with the stock train-mode backbone, with the fused one (bev_train.py:
csrc/bn_train.hip BatchNorm + ReLU, Winograd stride-1 convolutions forward and input gradient, weight gradients on the library),
with the fused one + wgrad="wino" (csrc/wino43_wgrad.hip for the stride-1 3x3 weight gradients) and with that + deblock="gemm"
(csrc/deconv_gemm.hip / csrc/deconv_train.hip for the deblocks' up-convolutions, forward and both gradients), alternated in one
process:

  step      PointPillarKITTI.train_loss(backbone=...) + backward (gradients of every parameter);
  backbone  backbone_head_stock / backbone_head_train + backward alone on a fixed channels-last canvas (no PFN, scatter or loss).

Inputs: 16 synthetic KITTI-like clouds and boxes (tests/_pp_train_torch.py's workload).  Device events (_measure.alternate), each iteration times
one call of each column back to back; medians after warm-up; peak memory from torch.cuda.max_memory_allocated above what was
allocated before the call.  Prints one JSON line.

  python tools/bev_train_bench.py [--iters 20] [--only stock|fused|fused_wino|fused_wino_gemm] [--rocprof OUTDIR]

--rocprof OUTDIR: afterwards runs this script once more per column in child processes (--only stock, fused, fused_wino, fused_wino_gemm) under
`rocprofv3 --kernel-trace --stats --output-format csv -d OUTDIR/<column>` (kernel trace only, no counters), so each column's kernel
statistics come from a run of their own.
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

import _pp_train_torch as T  # noqa: E402
from _measure import alternate, peak_mb  # noqa: E402


KINDS = ("stock", "fused", "fused_wino", "fused_wino_gemm")
# column -> (backbone option, wgrad option, deblock option) of PointPillarKITTI.train_loss / backbone_head_train
OPTIONS = {"stock": ("stock", "library", "library"), "fused": ("fused", "library", "library"), "fused_wino": ("fused", "wino", "library"),
           "fused_wino_gemm": ("fused", "wino", "gemm")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=KINDS, default=None)
    ap.add_argument("--rocprof", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bev_train_bench: no GPU")
    from lidardetection_amd.pointpillar import PointPillarKITTI
    dev, B = T.DEV, 16
    pts, offs, gt = T.pp_inputs(B, 5)
    torch.manual_seed(4)
    pp = PointPillarKITTI(batch_size=B, device=dev).train()
    params = [p for p in pp.parameters() if p.requires_grad]
    bev_params = [p for m in (pp.blocks, pp.deblocks, pp.conv_cls, pp.conv_box, pp.conv_dir_cls) for p in m.parameters()]
    g = torch.Generator(device="cpu").manual_seed(1)
    canvas = torch.relu(torch.randn(B, 64, pp.ny, pp.nx, generator=g)).to(dev).contiguous(memory_format=torch.channels_last)
    heads_g = None

    def step(kind):
        bb, wg, de = OPTIONS[kind]
        return lambda: torch.autograd.grad(sum(pp.train_loss(pts, offs, gt, backbone=bb, wgrad=wg, deblock=de)), params)

    def backbone(kind):
        def run():
            nonlocal heads_g
            head = pp.backbone_head_stock(canvas) if kind == "stock" else pp.backbone_head_train(canvas, *OPTIONS[kind][1:])
            if heads_g is None:
                heads_g = [torch.randn(h.shape, generator=g).to(dev) for h in head]
            torch.autograd.grad(sum((h * hg).sum() for h, hg in zip(head, heads_g)), bev_params)
        return run

    kinds = [args.only] if args.only else list(KINDS)
    result = {"tool": "bev_train_bench", "device": torch.cuda.get_device_name(0), "batch": B}
    for name, make in (("backbone", backbone), ("step", step)):
        fns = {k: make(k) for k in kinds}
        t = alternate(fns, args.iters, 3)
        w = {}
        for k in kinds:
            w.update({f"{k}_ms_median": round(t[k][0], 3), f"{k}_ms_min": round(t[k][1], 3), f"{k}_peak_mb": peak_mb(fns[k])})
        if len(kinds) == len(KINDS):
            w["speedup"] = round(t["stock"][0] / t["fused"][0], 3)
            w["wino_wgrad_speedup"] = round(t["fused"][0] / t["fused_wino"][0], 3)        # over the fused column (wgrad="library")
            w["gemm_deblock_speedup"] = round(t["fused_wino"][0] / t["fused_wino_gemm"][0], 3)   # over fused_wino (deblock="library")
        result[name] = w
    print(json.dumps(result), flush=True)
    if args.rocprof:
        for k in KINDS:
            # `timeout -k 10` bounds the whole process group, the profiled Python child included
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
                   os.path.join(args.rocprof, k), "-o", "bev_train", "--", sys.executable, os.path.abspath(__file__), "--only", k,
                   "--iters", "5"]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(f"bev_train_bench: rocprofv3 pass ({k}) exited with {rc}")


if __name__ == "__main__":
    main()
