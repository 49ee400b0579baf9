"""PV-RCNN-shaped micro-benchmarks (BASELINE.json configs[3], bs 8, ring clouds): FPS keypoints, stacked ball query +
grouping (VoxelSetAbstraction radii), 3-NN + interpolation, RoI-aware pooling, RoI-grid ball query, RoI-point pooling,
points-in-boxes.  Rates are the ones SURVEY §8d names (distance tests/s, gathered bytes/s, FPS latency per sample)."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd import synth
from lidardetection_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pn_stack
from lidardetection_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pn_batch
from lidardetection_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as roiaware
from lidardetection_amd.pcdet.ops.roipoint_pool3d import roipoint_pool3d_utils as roipoint
from _measure import event_total_ms

dev = torch.device("cuda:0")
B, NKP, NROI = 8, 2048, 128


def timeit(fn, n=10):
    return event_total_ms(fn, n, 3) * 1e3      # us per call


frames = [synth.cloud_ring(2000 + f)[:19968] for f in range(B)]
N = min(len(f) for f in frames)
pts = torch.from_numpy(np.stack([f[:N] for f in frames])).to(dev)                 # (B, N, 4)
xyz_b = pts[..., :3].contiguous()
with torch.no_grad():
    t = timeit(lambda: pn_batch.furthest_point_sample(xyz_b, NKP))
    print(f"FPS  {B} x {N} pts -> {NKP} keypoints: {t:8.1f} us  ({t / NKP * 1e3:.0f} ns per sample round, "
          f"{B * (NKP - 1) * N / t / 1e3:.1f} G distance updates/s)")
    kp_idx = pn_batch.furthest_point_sample(xyz_b, NKP).long()
    kp = torch.gather(xyz_b, 1, kp_idx.unsqueeze(-1).expand(-1, -1, 3))           # (B, NKP, 3)
    xyz = xyz_b.reshape(-1, 3).contiguous(); xyz_cnt = torch.full((B,), N, dtype=torch.int32, device=dev)
    new_xyz = kp.reshape(-1, 3).contiguous(); new_cnt = torch.full((B,), NKP, dtype=torch.int32, device=dev)
    C = 32
    feats = torch.randn(B * N, C, device=dev)
    for radius, ns in ((0.4, 16), (0.8, 16), (1.2, 32), (2.4, 32)):
        t = timeit(lambda: pn_stack.ball_query(radius, ns, xyz, xyz_cnt, new_xyz, new_cnt))
        idx, _ = pn_stack.ball_query(radius, ns, xyz, xyz_cnt, new_xyz, new_cnt)
        tg = timeit(lambda: pn_stack.grouping_operation(feats, xyz_cnt, idx, new_cnt))
        print(f"ball query r={radius} ns={ns}: M={B * NKP} x N_b={N}: {t:7.1f} us ({B * NKP * N / t / 1e3:.1f} G tests/s upper bound) | "
              f"group C={C}: {tg:7.1f} us ({B * NKP * C * ns * 4 * 2 / tg / 1e3:.1f} GB/s gathered+written)")
    t = timeit(lambda: pn_stack.three_nn(xyz, xyz_cnt, new_xyz, new_cnt))
    d, i3 = pn_stack.three_nn(xyz, xyz_cnt, new_xyz, new_cnt)
    w = (1.0 / (d + 1e-8)); w = (w / w.sum(1, keepdim=True)).contiguous()
    kf = torch.randn(B * NKP, 128, device=dev)
    ti = timeit(lambda: pn_stack.three_interpolate(kf, i3, w))
    print(f"3-NN {B * N} unknown x {NKP} known/frame: {t:7.1f} us ({B * N * NKP / t / 1e3:.1f} G tests/s) | interpolate C=128: {ti:7.1f} us")
    rois = torch.from_numpy(np.stack([synth.boxes_random(4000 + f, NROI) for f in range(B)])).to(dev)    # (B, NROI, 7)
    pf = torch.randn(N, 128, device=dev)
    pool = roiaware.RoIAwarePool3d(out_size=14, max_pts_each_voxel=128)
    t = timeit(lambda: pool(rois[0], xyz_b[0].contiguous(), pf, pool_method='max'))
    print(f"roiaware_pool3d 1 frame: {NROI} rois x {N} pts, 14^3 x 128 ch (max): {t:7.1f} us")
    t = timeit(lambda: roiaware.points_in_boxes_gpu(xyz_b, rois))
    print(f"points_in_boxes_gpu {B} x {N} pts x {NROI} boxes: {t:7.1f} us ({B * N * NROI / t / 1e3:.1f} G tests/s)")
    rp = roipoint.RoIPointPool3d(num_sampled_points=512, pool_extra_width=(1.0, 1.0, 1.0))
    pfb = torch.randn(B, N, 128, device=dev)
    t = timeit(lambda: rp(xyz_b, pfb, rois))
    print(f"roipoint_pool3d {B} x {NROI} rois x {N} pts -> 512 samples x (3+128): {t:7.1f} us")
    grid = torch.randn(B * NROI * 216, 3, device=dev) * 0.5 + new_xyz[:1]                     # 6^3 grid points per roi
    gcnt = torch.full((B,), NROI * 216, dtype=torch.int32, device=dev)
    t = timeit(lambda: pn_stack.ball_query(0.8, 16, new_xyz, new_cnt, grid.contiguous(), gcnt))
    print(f"roi-grid ball query r=0.8 ns=16: M={B * NROI * 216} x {NKP} keypoints: {t:7.1f} us ({B * NROI * 216 * NKP / t / 1e3:.1f} G tests/s)")
