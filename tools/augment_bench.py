"""Times the train-time augmentation (lidardetection_amd/augment.py, csrc/augment.hip) on a synthetic KITTI-like batch: 16 frames of
about 19 000 points, 15 candidates in each of 3 groups, road plane, sample rotation, flip / rotation / scaling.  Reports
  * the device time of one lidar_augment call (its five launches), from events around a run of calls on one stream;
  * the wall time of TrainAugmentor.__call__ (host draws, uploads, allocation and the launches), with a synchronise at the end;
  * the time of tests/_augment_np.py, the numpy restatement of the same contract, on one CPU for the same batch;
  * the algorithmic bytes (every input, object and output row once) over the device time, against 8 TB/s.
One JSON line.  Usage: python tools/augment_bench.py [--batch 16] [--iters 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _augment_np as anp  # noqa: E402
from lidardetection_amd import _lib, augment  # noqa: E402
from _measure import event_total_ms, host_ms  # noqa: E402


def make_batch(B, seed=0, G=3, S=15, n_db=600, M=24):
    r = np.random.default_rng(seed)
    F = np.float32
    side = int(np.ceil(np.sqrt(n_db)))
    boxes = np.zeros((n_db, 7), F)
    for i, cell in enumerate(r.permutation(side * side)[:n_db]):
        boxes[i] = [3 + 64.0 / side * (cell % side), -38 + 76.0 / side * (cell // side), r.uniform(-1.2, -0.6), r.uniform(1.5, 4.0),
                    r.uniform(0.6, 1.7), r.uniform(1.4, 1.8), r.uniform(-np.pi, np.pi)]
    sizes = r.integers(20, 400, n_db)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    dbp = np.concatenate([r.uniform(-0.5, 0.5, (offs[-1], 3)) * np.repeat(boxes[:, 3:6], sizes, axis=0), r.uniform(0, 1, (offs[-1], 1))], 1).astype(F)
    frame_points = r.integers(18000, 20001, B)
    n = int(frame_points.sum())
    pts = np.concatenate([np.stack([r.uniform(-2, 72, n), r.uniform(-42, 42, n), r.uniform(-2.2, 0.4, n)], 1), r.uniform(0, 1, (n, 1))], 1).astype(F)
    gt = np.zeros((B, M, 8), F)
    counts = r.integers(3, 13, B).astype(np.int32)
    cand = np.zeros((B, G, S), np.int32)
    for b in range(B):
        cand[b] = r.permutation(n_db)[:G * S].reshape(G, S)
        for j in range(counts[b]):
            gt[b, j] = [r.uniform(4, 66), r.uniform(-36, 36), -0.9, 3.9, 1.6, 1.56, r.uniform(-np.pi, np.pi), 1 + j % 3]
    inp = dict(points=pts, point_offsets=np.concatenate([[0], np.cumsum(frame_points)]).astype(np.int32), gt_boxes=gt, gt_counts=counts,
               db_points=dbp, db_offsets=offs, db_boxes=boxes, db_cls=r.integers(1, 4, n_db).astype(np.int32), cand=cand,
               flip_x=r.integers(0, 2, B).astype(np.int32), flip_y=np.zeros(B, np.int32), rot=r.uniform(-0.785, 0.785, B).astype(F),
               scale=r.uniform(0.95, 1.05, B).astype(F), sample_rot=r.uniform(-0.3, 0.3, (B, G, S)).astype(F),
               plane=np.stack([[r.normal(0, 0.01), r.normal(0, 0.01), r.normal(0, 0.01), r.uniform(-1.8, -1.5)] for _ in range(B)]).astype(F))
    cfg = dict(remove_extra_width=[0.0, 0.0, 0.0], collide_extra_width=None, pc_range=anp.KITTI_RANGE, remove_outside_boxes=True,
               min_num_corners=1, apply_scale=True)
    return inp, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = "cuda:0"
    inp, cfg = make_batch(args.batch)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    db = augment.GtDatabase(inp["db_points"], inp["db_offsets"], inp["db_boxes"], inp["db_cls"], device=dev)
    aug = augment.TrainAugmentor(db, 3, cfg["pc_range"], remove_extra_width=cfg["remove_extra_width"], sample_rot_range=(-0.3, 0.3))
    dargs = [up(inp[k]) for k in ("points", "point_offsets", "gt_boxes", "gt_counts")]
    kw = dict(planes=inp["plane"], flip_x=inp["flip_x"], flip_y=inp["flip_y"], rot=inp["rot"], scale=inp["scale"], sample_rot=inp["sample_rot"])
    out = aug(*dargs, inp["cand"], **kw)
    torch.cuda.synchronize()
    # the restatement on one CPU, and agreement of the counts (the inputs are not drawn clear of the thresholds: a count may differ by a row)
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    ref = anp.augment(inp, cfg)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    offs = out["point_offsets"].cpu().numpy()
    rows_off = int(np.abs(offs - ref["point_offsets"]).max())
    # wrapper wall time
    wrapper_ms = host_ms(lambda: aug(*dargs, inp["cand"], **kw), args.iters, warmup=args.warmup)
    # the raw call, device time from events
    L = _lib.lib()
    B, G, S = inp["cand"].shape
    M, n = inp["gt_boxes"].shape[1], inp["points"].shape[0]
    cap = int(out["points"].shape[0])
    rot64 = inp["rot"].astype(np.float64)
    d = {k: up(inp[k]) for k in ("cand", "flip_x", "flip_y", "rot", "scale", "sample_rot", "plane")}
    cs = up(np.stack([np.cos(rot64), np.sin(rot64)], 1).astype(np.float32))
    o = {k: torch.empty_like(v) for k, v in out.items() if torch.is_tensor(v)}
    ws = torch.empty(int(L.lidar_augment_workspace_bytes(B, G, S, cap)), dtype=torch.uint8, device=dev)
    rw, rng = _lib.host_f32(cfg["remove_extra_width"]), _lib.host_f32(cfg["pc_range"])

    def call():
        return L.lidar_augment(_lib.ptr(dargs[0]), _lib.ptr(dargs[1]), n, 4, _lib.ptr(dargs[2]), _lib.ptr(dargs[3]), B, M, _lib.ptr(db.points),
                               _lib.ptr(db.offsets), _lib.ptr(db.boxes), _lib.ptr(db.cls), db.n_obj, int(db.points.shape[0]), _lib.ptr(d["cand"]),
                               G, S, _lib.ptr(d["flip_x"]), _lib.ptr(d["flip_y"]), _lib.ptr(d["rot"]), _lib.ptr(cs), _lib.ptr(d["scale"]),
                               _lib.ptr(d["sample_rot"]), _lib.ptr(d["plane"]), rw, None, rng, 1, 1, cap - n, cap, _lib.ptr(o["points"]),
                               _lib.ptr(o["point_offsets"]), _lib.ptr(o["gt_boxes"]), _lib.ptr(o["gt_counts"]), _lib.ptr(o["sample_valid"]),
                               _lib.ptr(ws), ws.numel(), _lib.stream())

    for _ in range(args.warmup):
        assert call() == 0
    times = [event_total_ms(call, args.iters, 0) for _ in range(5)]
    assert torch.equal(o["points"][:int(offs[-1])], out["points"][:int(offs[-1])])
    dev_ms = float(np.median(times))
    pasted = int(np.where(out["sample_valid"].cpu().numpy() > 0, np.diff(inp["db_offsets"])[inp["cand"]], 0).sum())
    algo_bytes = (n + pasted + int(offs[-1])) * 4 * 4
    print(json.dumps(dict(
        bench="augment", batch=B, points_in=n, points_out=int(offs[-1]), candidates=int(G * S), samples_valid=int(out["sample_valid"].sum()),
        pasted_points=pasted, device_ms_per_call=round(dev_ms, 4), device_ms_runs=[round(t, 4) for t in times],
        wrapper_wall_ms_per_call=round(wrapper_ms, 4), numpy_one_cpu_ms=round(cpu_ms, 1), algorithmic_bytes=algo_bytes,
        achieved_GBps=round(algo_bytes / dev_ms / 1e6, 1), share_of_8TBps=round(algo_bytes / dev_ms / 1e6 / 8000, 4),
        hbm_floor_us=round(algo_bytes / 8e12 * 1e6, 2), offsets_max_row_difference_vs_numpy=rows_off, device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
