"""Times the tail of a PointPillar-KITTI training step, stock against fused, on the model's real parameter list with random
gradients (no forward or backward pass runs):

  stock: clip_grad_norm_ + the p.data.mul_(1 - wd * lr) loop + torch.optim.Adam.step()   (the reference's adam_onecycle tail)
  fused: lidardetection_amd.optim.AdamOneCycle.step()                                    (csrc/optim_step.hip, three launches)

For each: GPU time per step from device events around the whole window, and host enqueue time per step (host clock from the first
call to the return of the last, nothing synchronised in between; the queue is drained before the window starts).  The two are
measured in alternating windows of the same process.  Also printed: the algorithmic bytes of the fused step (16 B read + 16 B
written per element with the clipped gradient stored back, norm pass 4 B read) over its GPU time, as a fraction of the 8.0 TB/s
HBM peak.  One JSON line.

Usage: python tools/optim_step_bench.py [--steps 100] [--warmup 20] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch
from torch.nn.utils import clip_grad_norm_

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd import optim  # noqa: E402
from lidardetection_amd.pointpillar import PointPillarKITTI  # noqa: E402

from _measure import event_and_enqueue_ms  # noqa: E402

HBM_PEAK = 8.0e12
WD, CLIP = 0.01, 10.0


def timed(fn, steps):
    """-> (GPU ms per step, host enqueue ms per step) of `steps` calls of fn(i)"""
    it = iter(range(steps))
    return event_and_enqueue_ms(lambda: fn(next(it)), steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench needs the GPU: a CPU run measures nothing")
    dev = "cuda:0"
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(PointPillarKITTI(batch_size=2, device=dev).train())
    stock_model, fused_model = models
    stock_params = [p for p in stock_model.parameters() if p.requires_grad]
    fused = optim.AdamOneCycle(fused_model, wd=WD, max_grad_norm=CLIP)
    gen = torch.Generator(device=dev).manual_seed(1)
    for ps in (stock_params, fused.params):
        for p in ps:
            p.grad = torch.empty_like(p).normal_(generator=gen) * 0.01
    adam = torch.optim.Adam(stock_params, lr=0.0, betas=(0.9, 0.99))
    total = args.warmup + args.rounds * args.steps + 1

    def stock_step(i):
        lr, mom = optim.one_cycle(i % total, total)
        clip_grad_norm_(stock_params, CLIP)
        for p in stock_params:
            p.data.mul_(1 - WD * lr)
        for g in adam.param_groups:
            g["lr"], g["betas"] = lr, (mom, 0.99)
        adam.step()

    def fused_step(i):
        fused.lr, fused.mom = optim.one_cycle(i % total, total)
        fused.step()

    timed(stock_step, args.warmup)
    timed(fused_step, args.warmup)
    rows = {"stock": [], "fused": []}
    for _ in range(args.rounds):                     # alternate, so that a drift of the machine hits both
        rows["stock"].append(timed(stock_step, args.steps))
        rows["fused"].append(timed(fused_step, args.steps))
    numel = sum(p.numel() for p in fused.params)
    best = {k: (min(r[0] for r in v), min(r[1] for r in v)) for k, v in rows.items()}
    bytes_step = numel * (4 + 16 + 16)               # norm pass reads g; update reads p, g, m, v and writes p, g, m, v
    out = {"metric": "PointPillar-KITTI optimiser tail, ms per step (best of rounds)", "tensors": len(fused.params), "numel": numel,
           "chunks": fused._n_chunks, "steps": args.steps, "rounds": args.rounds,
           "stock_gpu_ms": best["stock"][0], "stock_host_enqueue_ms": best["stock"][1],
           "fused_gpu_ms": best["fused"][0], "fused_host_enqueue_ms": best["fused"][1],
           "all_rounds": rows, "fused_algorithmic_bytes": bytes_step,
           "fused_fraction_of_hbm_peak": bytes_step / (best["fused"][0] * 1e-3) / HBM_PEAK}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
