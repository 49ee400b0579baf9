"""bench.py — frames/s of PointPillar-KITTI forward + NMS (BASELINE.json metric) on N MI355X.

Step  = one pass of the hot path over one batch of 16 synthetic KITTI-shaped frames resident in HBM:
        HIP voxelise -> HIP PillarVFE -> dense 2D backbone + head in fp32 (r04: first layer from the pillars, Winograd 3x3 layers and
        fused deblocks are this repo's MFMA kernels; two stride-2 layers MIOpen, stride-1 deblock + heads hipBLASLt)
        -> exact top-k + decode -> HIP batched rotated NMS (device greedy).
N > 1 = one process per GPU (torch.distributed / RCCL only for the barrier + max-over-ranks
        timing); frames are independent, every rank processes its own batch: replicas, weak scaling,
        no data-path collective.

Prints ONE JSON line on rank 0: metric / value / unit / higher_is_better / dtype / ms_per_step of the --steps timed steps.
A plain run does only that (set up, warm up, time, optionally --dump-outputs, print).  --full adds, after the timed steps:
  roofline     — the voxeliser (the north-star HBM kernel sequence), timed with HIP events on the
                 launch stream inside the timed region; algorithmic bytes per launch from SURVEY §8d.
  extra        — side measurements (tools/bench_extra.py: H2D-inclusive rate, SECOND / sparse GEMM / NMS / PFN, ...).
  cpu_baseline — the oracle (CPU restatement of the reference path) timed on a bounded sample.

--dump-outputs DIR writes what the last timed step returned (rank 0): boxes, scores (float32), labels, counts (float64, exact)
as DIR/<name>.npy.  Inputs and weights are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from lidardetection_amd import dist_utils, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def make_batch(batch, rank, device):
    frames = [synth.cloud_uniform(1000 + rank * batch + f) for f in range(batch)]
    sizes = [len(f) for f in frames]
    pts = torch.from_numpy(np.concatenate(frames, 0)).to(device)
    hoffs = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]       # the collate step knows the offsets on the host too
    offs = torch.tensor(hoffs, dtype=torch.int32, device=device)
    return frames, pts, offs, hoffs, max(sizes)


def _hot_path_stages_cpu(frame, boxes, w, bn, max_voxels, nms_thresh, clk=time.perf_counter):
    """one frame through the reference's CPU hot path, restated (oracle/): -> seconds per stage"""
    from oracle import c_oracle, pp_oracle
    a = clk()
    vox, coords, num = c_oracle.voxelize(frame, synth.PP_VOXEL, synth.PP_RANGE, 32, max_voxels)
    t_vox = clk() - a
    coords4 = torch.from_numpy(np.pad(coords, ((0, 0), (1, 0)))).float()
    with torch.no_grad():
        a = clk()
        feat = pp_oracle.pillar_vfe(torch.from_numpy(vox), torch.from_numpy(num).float(), coords4, w, *bn, synth.PP_VOXEL, synth.PP_RANGE, eps=1e-3)
        pp_oracle.pillar_scatter(feat, coords4, 1, 432, 496)
        t_pfn = clk() - a
    a = clk()
    c_oracle.nms_sorted(boxes, nms_thresh)
    return t_vox, t_pfn, clk() - a


def _cpu_worker(args):
    """one process of the one-process-per-core column (spawned; never touches the GPU): `nfr` frames after one warm-up"""
    seed, nfr, max_voxels, nms_thresh = args
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 10, generator=g) * 0.3
    bn = (torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2, torch.zeros(64), torch.ones(64))
    b, sc = synth.boxes_nms(seed=3000 + seed)
    boxes = np.ascontiguousarray(b[np.argsort(-sc, kind="stable")])
    frames = [synth.cloud_uniform(1000 + seed * 7 + k) for k in range(nfr + 1)]
    _hot_path_stages_cpu(frames[0], boxes, w, bn, max_voxels, nms_thresh)
    t0 = time.perf_counter()
    for f in frames[1:]:
        _hot_path_stages_cpu(f, boxes, w, bn, max_voxels, nms_thresh)
    return time.perf_counter() - t0


def _cpu_share():
    """CPUs this process may really use: affinity mask and cgroup quota, capped at 16 (a one-GPU box's share of its host)"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return max(1, min(n, 16))


def cpu_baseline(frames, model, nframes, nruns=20, warmups=3, procs_cap=16):
    """the reference's CPU hot path restated (oracle/): sequential voxelise (C, 1 thread) + PillarVFE /
    PointPillarScatter (torch CPU) + rotated NMS on the SURVEY 8d clustered set (C, 1 thread).  3 warm-ups, >= 20 timed runs per
    column, median and p10 / p90 per stage; columns: single-thread latency, one process with set_num_threads(nproc), one
    single-threaded process per core (capped).  `value` = end-to-end frames/s incl. the torch-CPU dense backbone + head on a
    short sample (it is the other 40 % of a CPU frame and not part of the section-5 protocol)."""
    from oracle import c_oracle
    import copy
    import multiprocessing as mp
    nproc = _cpu_share()
    try:
        cpu_model = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")][0]
    except Exception:
        cpu_model = "unknown"
    keep = (model._bev, model._canvas)      # device-side folded weights / concat + canvas buffers: not part of the host copy
    model._bev = model._canvas = None
    m = copy.deepcopy(model).to("cpu")
    model._bev, model._canvas = keep
    m.B = 1
    m.fold_bn = False           # the HIP epilogue has no CPU path: stock modules on the host
    m.anchors = m.anchors.cpu()
    n_ = m.pfn_norm
    w = m.pfn_linear.weight.detach()
    bn = (n_.weight.detach(), n_.bias.detach(), n_.running_mean, n_.running_var)
    b, sc = synth.boxes_nms(seed=3000)
    boxes = np.ascontiguousarray(b[np.argsort(-sc, kind="stable")])
    pct = lambda a: {"median": float(np.median(a)) * 1e3, "p10": float(np.percentile(a, 10)) * 1e3, "p90": float(np.percentile(a, 90)) * 1e3}
    t_begin = time.perf_counter()

    def column(threads):
        torch.set_num_threads(threads)
        rows = [_hot_path_stages_cpu(frames[k % len(frames)], boxes, w, bn, model.voxelizer.max_voxels, model.nms_thresh)
                for k in range(warmups + nruns)][warmups:]
        a = np.asarray(rows)
        return {"voxelize_ms": pct(a[:, 0]), "pfn_scatter_ms": pct(a[:, 1]), "nms_ms": pct(a[:, 2]),
                "frames_per_s": float(1.0 / np.median(a.sum(1)))}

    keep_threads = torch.get_num_threads()
    single = column(1)
    allthr = column(nproc)
    # one single-threaded process per core (spawned before nothing: the children import torch on the CPU only)
    P = max(1, min(nproc, procs_cap))
    per_core = None
    try:
        env_keep = os.environ.get("HIP_VISIBLE_DEVICES")
        os.environ["HIP_VISIBLE_DEVICES"] = ""            # inherited by the children: no GPU initialisation there
        with mp.get_context("spawn").Pool(P) as pool:
            t0 = time.perf_counter()
            secs = pool.map(_cpu_worker, [(k, 3, model.voxelizer.max_voxels, model.nms_thresh) for k in range(P)])
        per_core = {"processes": P, "frames_per_process": 3, "frames_per_s": float(3 * P / max(secs)),
                    "note": "hot-path stages only; wall time of the slowest process, process start-up excluded"}
    except Exception as e:      # the checker must never sink the measurement
        per_core = {"processes": P, "error": repr(e)[:160]}
    finally:
        if env_keep is None:
            os.environ.pop("HIP_VISIBLE_DEVICES", None)
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = env_keep
    # end to end on a short sample, all threads: hot path + dense backbone + head + decode
    torch.set_num_threads(nproc)
    st = {"voxelize": 0.0, "pfn_scatter": 0.0, "backbone_head": 0.0, "post_decode": 0.0, "nms": 0.0}
    clk = time.perf_counter
    from oracle import pp_oracle
    t0 = clk()
    for f in frames[:nframes]:
        a = clk()
        vox, coords, num = c_oracle.voxelize(f, synth.PP_VOXEL, synth.PP_RANGE, 32, model.voxelizer.max_voxels)
        st["voxelize"] += clk() - a
        coords4 = torch.from_numpy(np.pad(coords, ((0, 0), (1, 0)))).float()
        with torch.no_grad():
            a = clk()
            feat = pp_oracle.pillar_vfe(torch.from_numpy(vox), torch.from_numpy(num).float(), coords4, w, *bn, synth.PP_VOXEL, synth.PP_RANGE, eps=n_.eps)
            canvas = pp_oracle.pillar_scatter(feat, coords4, 1, m.nx, m.ny)
            st["pfn_scatter"] += clk() - a
            a = clk()
            cls, box, dirs = m.backbone_head(canvas)
            st["backbone_head"] += clk() - a
            a = clk()
            scores, _ = torch.sigmoid(cls[0]).max(dim=-1)
            msk = scores >= m.score_thresh
            sc2, idx = torch.topk(scores[msk], k=min(m.nms_pre, int(msk.sum())))
            oi = msk.nonzero().view(-1)[idx]
            bx = m.decode(box[0][oi], m.anchors[oi], dirs[0][oi])
            st["post_decode"] += clk() - a
        a = clk()
        c_oracle.nms_sorted(bx.numpy(), m.nms_thresh)
        st["nms"] += clk() - a
    dt = clk() - t0
    torch.set_num_threads(keep_threads)
    return {"value": nframes / dt, "unit": "frames/s", "cores": nproc, "kind": "port", "cpu_model": cpu_model, "nproc": nproc, "host_cpus": os.cpu_count(),
            "protocol": f"BASELINE.md section 5: {warmups} warm-ups, {nruns} timed runs per column, median / p10 / p90 per stage",
            "hot_path_single_thread": single, "hot_path_one_process_all_threads": dict(allthr, torch_threads=nproc),
            "hot_path_one_process_per_core": per_core,
            "stage_ms_per_frame": {k: v / nframes * 1e3 for k, v in st.items()},
            "sample": f"value: {nframes} frame(s) end to end (C oracle voxelise + NMS 1 thread each, torch-CPU PFN / scatter / backbone / head "
                      f"with {nproc} threads), {dt:.1f} s; hot-path columns: {warmups}+{nruns} frames each; whole baseline {clk() - t_begin:.0f} s"}


def h2d_inclusive(model, frames, steps, device, resident_fps):
    """the same step with the raw clouds arriving from HOST memory every step — copied into pinned staging,
    H2D on a side stream, overlapped with the previous step (lidardetection_amd/feeder.py).  `value` stays the resident figure;
    this is the PCIe-inclusive one beside it."""
    from lidardetection_amd.feeder import PinnedPointFeeder
    B = len(frames)
    feeder = PinnedPointFeeder(sum(len(f) for f in frames), frames[0].shape[1], max_batch=B, device=device, depth=2)
    with torch.no_grad():
        feeder.submit(frames)
        for _ in range(3):
            feeder.submit(frames)
            fb = feeder.get()
            model(fb.points, fb.offsets, fb.host_offsets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            feeder.submit(frames)                   # next batch: host copy into pinned memory + async H2D, under this step's kernels
            fb = feeder.get()
            model(fb.points, fb.offsets, fb.host_offsets)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        feeder.get()
    fps = B * steps / dt
    return {"h2d_inclusive_frames_per_s": fps, "h2d_inclusive_ms_per_step": dt / steps * 1e3, "h2d_inclusive_vs_resident": fps / resident_fps,
            "h2d_bytes_per_step": int(sum(f.nbytes for f in frames)),
            "h2d_note": "raw (N, 4) clouds from host numpy arrays every step: pinned double-buffered staging + copy stream (feeder.py)"}


def dump_outputs(out_dir, out):
    """what a caller of the timed path receives from its last step: boxes (B, post, 7), scores (B, post), labels (B, post),
    counts (B) -> out_dir/<name>.npy; float32 as computed, the integer arrays as float64 (exact)"""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in zip(("boxes", "scores", "labels", "counts"), out):
        a = t.detach().cpu().numpy()
        a = a.astype(np.float32) if a.dtype == np.float32 else a.astype(np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a torch.distributed launcher: start N fresh rank processes, one per GPU, with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set (what tools/scripts/dist_train.sh:7 + pcdet/utils/common_utils.py:170-184
    do for the reference).  The parent never touches the GPU; it only waits and forwards the worst exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LIDAR_BENCH_CHILD="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def dry_run(args, rank, world):
    """--dry-run: the N-rank plumbing alone on CPU / gloo (launcher, rendezvous, barrier, max-over-ranks clock, the single
    JSON line) — no kernel is launched and nothing is measured."""
    dist = dist_utils.init_from_env("gloo")
    frames_of_rank = dist_utils.shard_indices(args.batch * world, rank, world)
    dist_utils.barrier(dist)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(1e-3)
    dist_utils.barrier(dist)
    dt = dist_utils.max_over_ranks(time.perf_counter() - t0, dist)
    if rank == 0:
        print(json.dumps({"metric": "frames/sec (fwd+NMS) PointPillar-KITTI", "value": None, "unit": "frames/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "dry_run": True,
                          "frames_per_rank": len(frames_of_rank), "scaling": "weak"}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=4)
    ap.add_argument("--no-extra", action="store_true", help="skip the SECOND / sparse-GEMM / NMS / PFN side measurements")
    ap.add_argument("--no-full-rewrite", action="store_true", help="skip the extra steps that time the non-resident voxeliser path "
                    "(profiles: keeps the per-kernel averages of the timed path unmixed)")
    ap.add_argument("--contract-only", action="store_true", help="run EVERY step (warm-up, timed, armed) on the voxeliser's contract path "
                    "(algo 3, fresh-buffer semantics: all priced bytes written) — profiles: a kernel trace of this run holds the "
                    "launches roofline.frac is priced on and nothing else under their names")
    ap.add_argument("--roofline-launches", type=int, default=100, help="armed launches behind roofline.ms_per_launch (SURVEY 8d: >= 100)")
    ap.add_argument("--mode", choices=["infer", "train-ddp"], default="infer", help="train-ddp: BASELINE configs[4]'s DDP leg — "
                    "SECOND-MultiHead NuScenes bs 4 / GPU, forward + backward + DistributedDataParallel step (tools/ddp_train_bench.py)")
    ap.add_argument("--dry-run", action="store_true", help="N-rank plumbing only, CPU / gloo, no kernels (tests)")
    ap.add_argument("--stages", action="store_true", help="also print per-stage GPU times (stderr); implies --full")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure the roofline, the `extra` side "
                    "measurements and the CPU baseline (the --no-* / --roofline-launches / --cpu-frames options apply here)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()
    args.full = args.full or args.stages

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))       # before anything touches the GPU
    rank, local, world = dist_utils.env_world()
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
              f"(torch.distributed.run --nproc-per-node {args.gpus}, or no launcher at all)", file=sys.stderr)
        sys.exit(2)
    if args.mode == "train-ddp":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import ddp_train_bench
        return ddp_train_bench.run(args, rank, local, world)
    if args.dry_run:
        return dry_run(args, rank, world)
    from lidardetection_amd.pointpillar import PointPillarKITTI
    if world > 1 and "MIOPEN_USER_DB_PATH" not in os.environ:
        # ONE user database for all ranks of this job: rank 0 runs MIOpen's find pass first (staged warm-up below) and records its
        # picks there; the other ranks then find those records instead of timing the candidates again, so that every rank runs the
        # same solver (N independent timing decisions could differ, and the max-over-ranks clock reports the unluckiest)
        import tempfile
        db = os.path.join(tempfile.gettempdir(), f"lidar_miopen_udb_{os.getuid()}_{os.environ.get('MASTER_PORT', '0')}")
        os.makedirs(db, exist_ok=True)
        os.environ["MIOPEN_USER_DB_PATH"] = db
    torch.cuda.set_device(local)
    dist = dist_utils.init_from_env("nccl")          # RCCL on ROCm; None for a single process
    device = torch.device("cuda", local)
    # MIOpen find mode for the stock fp32 convolutions (default on: +3 %; LIDAR_BENCH_MIOPEN_FIND=0 = heuristic pick, which is
    # deterministic across ranks and runs)
    torch.backends.cudnn.benchmark = os.environ.get("LIDAR_BENCH_MIOPEN_FIND", "1") != "0"

    frames, pts, offs, hoffs, n_max = make_batch(args.batch, rank, device)
    torch.manual_seed(0)
    model = PointPillarKITTI(batch_size=args.batch, max_voxels=16000, n_max=n_max, device=device).randomize_for_bench(0)

    def barrier():
        dist_utils.barrier(dist, cuda=True)

    if args.contract_only:
        model.resident_voxels = False
    with torch.no_grad():
        # staged warm-up for N > 1: rank 0 first — its convolution find results land in the shared MIOpen user database and its
        # library-GEMM picks are broadcast (lidar_dense_gemm_export / import_choices) — then everybody else with those choices
        if world > 1 and rank == 0:
            for _ in range(args.warmup):
                out = model(pts, offs, hoffs)
            torch.cuda.synchronize()
        if world > 1:
            picks = [dist_utils.export_gemm_choices()] if rank == 0 else [None]
            dist.broadcast_object_list(picks, src=0)
            if rank != 0:
                dist_utils.import_gemm_choices(picks[0])
        for _ in range(args.warmup if not (world > 1 and rank == 0) else 1):
            out = model(pts, offs, hoffs)
        barrier()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        ev0 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        from lidardetection_amd import _lib as _lh
        Lh = _lh.lib()
        for a, b in ev + ev0:       # torch creates the HIP event lazily at the first record(): do that outside the timed region
            a.record()
            b.record()
        barrier()
        t0 = time.perf_counter()
        for k in range(args.steps):
            ev0[k][0].record()                      # empty bracket: what a HIP event pair costs by itself at this point
            ev0[k][1].record()
            ev[k][0].record()                       # same stream the kernels are launched on
            vox = model.voxelize(pts, offs, hoffs)
            ev[k][1].record()
            canvas = model.vfe_scatter(vox)
            out = model.post_process(*model.backbone_head(canvas))
        barrier()
        dt = time.perf_counter() - t0
    dt = dist_utils.max_over_ranks(dt, dist, device)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    frames_total = args.batch * args.steps * world
    res = {
        "metric": "frames/sec (fwd+NMS) PointPillar-KITTI", "value": frames_total / dt, "unit": "frames/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "PointPillar-KITTI bs=16 per GPU, fp32, eval BN folded: HIP voxelize + PFN; dense 2D backbone = first layer from the "
                               "pillars (sparse implicit GEMM), stride-1 3x3 layers as Winograd F(4x4,3x3) on the fp32 MFMA, strided deblocks as one "
                               "fused MFMA GEMM (all this repo's HIP), the two stride-2 3x3 layers MIOpen, stride-1 deblock + 1x1 heads hipBLASLt; exact "
                               "HIP top-k + decode + batched rotated NMS; cloud_uniform 20k pts/frame, 16k pillars/frame (max_voxels cap), NMS pre 4096 "
                               "/ post 500 / thr 0.01",
                   "frames_per_step": args.batch, "replicas": world},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(res))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # Voxeliser durations for the roofline: the kernels' own start / stop events (lidar_timer_*: hipExtLaunchKernel carries them, the
    # timestamps a kernel trace reports) on extra full detector steps AFTER the timed region, >= 100 launches per path, split into
    # first kernel / inter-kernel gap / last kernel.  The hipEventRecord bracket around the same call is measured on separate
    # extra steps with PLAIN launches (an event-carrying launch adds queue time of its own, which is what made the r03 bracket
    # read 54 us): bracket_ms = kernel span + one event pair + dispatch.
    import ctypes

    def armed_steps(n):
        tms = [Lh.lidar_timer_create() for _ in range(n)]
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        with torch.no_grad():
            model(pts, offs, hoffs)
            for (a, b), tm in zip(evs, tms):
                a.record()
                v2 = model.voxelize(pts, offs, hoffs, tm)
                b.record()
                model.post_process(*model.backbone_head(model.vfe_scatter(v2)))
            torch.cuda.synchronize()
        spans, parts = [], []
        buf = (ctypes.c_float * 3)()
        for tm in tms:
            ms = Lh.lidar_timer_elapsed_ms(tm)
            if ms >= 0 and Lh.lidar_timer_parts_ms(tm, buf) == 0:
                spans.append(ms)
                parts.append([buf[0], buf[1], buf[2]])
            Lh.lidar_timer_destroy(tm)
        pa = np.asarray(parts, np.float64)
        return {"ms": float(np.mean(spans)), "median_ms": float(np.median(spans)), "p10_ms": float(np.percentile(spans, 10)),
                "p90_ms": float(np.percentile(spans, 90)), "launches": len(spans), "first_kernel_us": float(pa[:, 0].mean() * 1e3),
                "gap_us": float(pa[:, 1].mean() * 1e3), "last_kernel_us": float(pa[:, 2].mean() * 1e3),
                "kernel_sum_us": float((pa[:, 0] + pa[:, 2]).mean() * 1e3),
                "bracket_armed_ms": float(np.mean([a.elapsed_time(b) for a, b in evs]))}

    def plain_bracket_steps(n):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        with torch.no_grad():
            model(pts, offs, hoffs)
            for a, b in evs:
                a.record()
                v2 = model.voxelize(pts, offs, hoffs)
                b.record()
                model.post_process(*model.backbone_head(model.vfe_scatter(v2)))
            torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) for a, b in evs]))

    n_arm = max(args.roofline_launches, 5)
    contract = resident = None
    contract_bracket_ms = None
    if args.contract_only:
        contract = armed_steps(n_arm)
        contract_bracket_ms = plain_bracket_steps(min(n_arm, 40))
    else:
        resident = armed_steps(n_arm)                 # the timed path (resident output)
        if getattr(model, "resident_voxels", False) and not args.no_full_rewrite:
            model.resident_voxels = False
            contract = armed_steps(n_arm)
            contract_bracket_ms = plain_bracket_steps(min(n_arm, 40))
            model.resident_voxels = True
            model(pts, offs, hoffs)
    vox_ms = (resident or contract)["ms"]
    contract_ms = contract["ms"] if contract else None
    vox_bracket_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))          # timed region: hipEventRecord bracket
    ev_overhead_ms = float(np.mean([a.elapsed_time(b) for a, b in ev0]))
    total_rows = int(vox["voxel_offsets"][-1].item())
    npts = int(offs[-1].item())
    P, C = 32, 4
    alg_bytes = 16 * npts + total_rows * (P * C * 4 + 16 + 4)          # 16N + V(4PC + 16 + 4): the drop-in contract
    # what the RESIDENT path has to move by its own definition: points once + the previous call's occupied slots cleared + this
    # call's occupied slots written (16 B each) + coords / counts (the 96 %-zero padding persists between calls)
    slots = int(vox["voxel_num_points"][:total_rows].sum().item())
    own_bytes = 16 * npts + 2 * 16 * slots + 20 * total_rows
    # HBM traffic of the same launch sequences: rocprofv3 PMC counters cannot be collected from inside this run, so the figures
    # come from the committed passes (profiles/rNN/voxelize_pmc.json) and are only reported when that file was taken from the
    # SAME kernel source (sha256 of csrc/voxelize.hip recorded beside it); otherwise null — never a stale number.
    traffic = {"full": None, "resident": None}
    traffic_src = None
    import glob
    import hashlib
    with open(os.path.join(ROOT, "lidardetection_amd", "csrc", "voxelize.hip"), "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "voxelize_pmc.json")), reverse=True):     # newest round first
        if args.batch != 16:
            break
        with open(pmc) as fh:
            rec = json.load(fh)
        if rec.get("kernel_source_sha256_16") == sha:
            traffic = {k: rec[k]["traffic_bytes_per_launch_high"] for k in ("full", "resident")}
            traffic_src = (f"{os.path.relpath(pmc, ROOT)} (voxelize.hip sha256 {sha}; FETCH_SIZE upper bracket + WRITE_SIZE, "
                           "separate --pmc passes)")
            break
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
    ratio = lambda tr, nbytes: None if tr is None else tr / nbytes
    # roofline.frac describes the path that MOVES the priced bytes: the drop-in contract (fresh output buffers, the whole padded
    # buffer rewritten, include/lidar_hip.h algo 3), bracketed with the same HIP events inside full steps right after the timed
    # region.  The timed region itself runs the resident-output mode (algo 4: same output bits, a quarter of the traffic); it is
    # reported under `timed_path` with the bytes IT has to move and, for comparison, the contract bytes over its time.
    # ms_per_launch = the two kernels' own durations (start -> stop events each launch carries), i.e. what `rocprofv3 --kernel-trace
    # --stats` reports as their average durations.  The SPAN of an event-carrying call also contains a 7-10 us gap between the
    # launches that plain launches do not have: in the kernel trace of this very command (profiles/r04/voxelize_contract_trace.json)
    # the plain launches' second kernel starts within 10 ns of the first one's end (gap 0.0 us) while the armed ones sit 7-10 us
    # apart — the completion signal + start timestamp of the events themselves.  So span_armed / gap_armed are reported, not priced.
    def roof_of(m, nbytes, path):
        ms = m["kernel_sum_us"] * 1e-3
        return {"achieved": gbs(nbytes, ms), "frac": gbs(nbytes, ms) / HBM_PEAK_GBS, "ms_per_launch": ms, "path": path}
    if contract is not None:
        roof = roof_of(contract, alg_bytes, "contract (algo 3, full rewrite), in-step, " +
                       ("every step of this run" if args.contract_only else "measured on extra steps after the timed region"))
    else:   # --no-full-rewrite: only the timed path was measured; price it with its own bytes
        roof = roof_of(resident, own_bytes, "resident (algo 4), in-step, extra steps after the timed region, priced with its own algorithmic bytes")
    vox_ms = (resident or contract)["kernel_sum_us"] * 1e-3
    res.update({
        "roofline": {"bound": "hbm", "kernel": "lidar_voxelize = vxl_keybin_kernel (bin + zero-fill roles in one launch) + vxl_emit_kernel",
                     "achieved": roof["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": roof["frac"], "path": roof["path"],
                     "ms_per_launch": roof["ms_per_launch"], "alg_bytes_per_launch": alg_bytes if contract_ms is not None else own_bytes,
                     # the same span split (means over `launches` armed launches): rocprofv3's per-kernel averages of this command
                     # (profiles/r04/) must agree with first_kernel_us / last_kernel_us, and ms_per_launch = their sum + gap_us
                     "launches": (contract or resident)["launches"], "kernel_sum_us": (contract or resident)["kernel_sum_us"],
                     "first_kernel_us": (contract or resident)["first_kernel_us"], "last_kernel_us": (contract or resident)["last_kernel_us"],
                     "gap_armed_us": (contract or resident)["gap_us"], "span_armed_ms": (contract or resident)["ms"],
                     "span_armed_p10_p90_ms": [(contract or resident)["p10_ms"], (contract or resident)["p90_ms"]],
                     "gap_plain_us_in_trace": "0.0 (profiles/r04/voxelize_contract_trace.json: same command under rocprofv3 --kernel-trace)",
                     "bracket_armed_ms_per_launch": (contract or resident)["bracket_armed_ms"],
                     "timing": "ms_per_launch = sum of the two kernels' own durations, each from the start / stop HIP events its launch carries "
                               "(hipExtLaunchKernel: the dispatch timestamps a kernel trace reports), mean over `launches` in-step launches; "
                               "span_armed_ms = first start to last end of those event-carrying calls (contains gap_armed_us, an artefact of "
                               "the events: plain launches run back to back in the trace); bracket_ms_per_launch = hipEventRecord before / after the call, "
                               "which adds the event-marker and queue overhead (event_pair_overhead_ms)",
                     "bracket_ms_per_launch": contract_bracket_ms if contract_ms is not None else vox_bracket_ms,
                     "traffic": traffic["full"] if contract_ms is not None else traffic["resident"],
                     "traffic_ratio": ratio(traffic["full"], alg_bytes) if contract_ms is not None else ratio(traffic["resident"], own_bytes),
                     "traffic_source": traffic_src,
                     # informational: an empty HIP event pair recorded at the same place (dispatch + marker latency that the
                     # brackets also contain); no `frac` subtracts it
                     "event_pair_overhead_ms": ev_overhead_ms,
                     "timed_path": {"mode": "resident output buffer (algo 4): the padded rows' zeros persist between calls, only the previous "
                                            "call's occupied slots are re-zeroed — same output bits as the contract path (tested)",
                                    "ms_per_launch": vox_ms, "bracket_ms_per_launch": vox_bracket_ms, "own_alg_bytes_per_launch": own_bytes,
                                    "kernel_sum_us": (resident or contract)["kernel_sum_us"], "gap_armed_us": (resident or contract)["gap_us"],
                                    "launches": (resident or contract)["launches"],
                                    "achieved_own": gbs(own_bytes, vox_ms), "frac_own": gbs(own_bytes, vox_ms) / HBM_PEAK_GBS,
                                    "equivalent_contract_frac": gbs(alg_bytes, vox_ms) / HBM_PEAK_GBS,
                                    "traffic": traffic["resident"], "traffic_ratio_vs_own": ratio(traffic["resident"], own_bytes),
                                    "traffic_ratio_vs_contract": ratio(traffic["resident"], alg_bytes)}},
    })
    if args.stages and rank == 0:
        def gpu_time(fn, n=20):
            """median GPU time of one call (per-call event pairs: a host-side pause between launches is not GPU time)"""
            for _ in range(2):
                r = fn()
            torch.cuda.synchronize()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in evs:
                a.record()
                r = fn()
                b.record()
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in evs])), r
        with torch.no_grad():
            tv, vox = gpu_time(lambda: model.voxelize(pts, offs, hoffs))
            ts, canvas = gpu_time(lambda: model.vfe_scatter(vox))
            tb, hb = gpu_time(lambda: model.backbone_head(canvas))
            tp, outp = gpu_time(lambda: model.post_process(*hb))
        print(f"[stages ms/batch] voxelize {tv:.3f} vfe+scatter {ts:.3f} backbone+head {tb:.3f} post+nms {tp:.3f} "
              f"kept/frame {outp[3].float().mean().item():.1f}", file=sys.stderr)
    if rank == 0 and world == 1 and not args.no_extra:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_extra
        del out, canvas, vox
        try:
            res["extra"] = h2d_inclusive(model, frames, args.steps, device, frames_total / world / dt)
        except Exception as e:
            res["extra"] = {"h2d_inclusive_error": repr(e)[:200]}
        try:
            res["extra"].update(bench_extra.pp_kernels(model, pts, offs))
            res["extra"].update(bench_extra.pp_ring(model))
            model(pts, offs, hoffs)
        except Exception as e:
            res["extra"] = dict(res.get("extra") or {}, pp_kernels_error=repr(e)[:200])
        torch.cuda.empty_cache()
        res["extra"].update(bench_extra.collect(device))
    if rank == 0:
        if not args.no_cpu_baseline and world == 1:
            try:
                res["cpu_baseline"] = cpu_baseline(frames, model, args.cpu_frames)
            except Exception as e:  # the checker must never sink the measurement
                res["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}
        print(json.dumps(res))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
