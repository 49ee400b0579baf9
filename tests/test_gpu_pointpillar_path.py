"""GPU parity of the PointPillar slice of the hot path (voxelise -> PFN -> scatter -> rotated NMS)
against the CPU oracle and the committed golden fixtures.  Calls go through the C ABI
(lidardetection_amd._lib -> liblidar_hip.so).  Bit-exact for integer / copied data; fp32 features
within the tolerance written at each assert (north_star: 1e-4)."""
import os

import numpy as np
import pytest
import torch

from lidardetection_amd import pillar_ops, synth
from lidardetection_amd.ext import iou3d_nms_cuda
from lidardetection_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
from lidardetection_amd.voxelizer import BatchVoxelizer
from oracle import c_oracle, pp_oracle

pytestmark = pytest.mark.gpu


def _check_voxel_parity(frames, vs, rng, P, maxv, C, dev, repeat=2):
    exp = [c_oracle.voxelize(f, vs, rng, P, maxv) for f in frames]
    ev, ec, en = pp_oracle.collate(exp)
    # both kernel paths: 3 = LDS-binned, 2 launches (default for n_max <= 32768), 2 = global hash
    for algo in (3, 2):
        _check_one_algo(frames, vs, rng, P, maxv, C, dev, repeat, algo, exp, ev, ec, en)


def _check_one_algo(frames, vs, rng, P, maxv, C, dev, repeat, algo, exp, ev, ec, en):
    vz = BatchVoxelizer(vs, rng, P, maxv, num_point_features=C, algo=algo)
    for _ in range(repeat):  # second pass proves the workspace restores itself
        out = vz.voxelize_frames(frames, device=dev)
        offs = out["voxel_offsets"].cpu().numpy()
        assert offs.tolist() == np.concatenate([[0], np.cumsum([len(e[0]) for e in exp])]).tolist()
        assert np.array_equal(out["voxel_coords"].cpu().numpy(), ec.astype(np.int32))
        assert np.array_equal(out["voxel_num_points"].cpu().numpy(), en)
        assert np.array_equal(out["voxels"].cpu().numpy().view(np.uint32), ev.view(np.uint32))


def test_voxelize_pointpillar_batch_bit_exact(dev):
    frames = [synth.cloud_ring(2000), synth.cloud_uniform(1000), synth.cloud_ring(2001)[:7777],
              np.zeros((0, 4), np.float32), synth.cloud_uniform(1001, n=333)]
    _check_voxel_parity(frames, synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4, dev)


def test_voxelize_shuffled_and_dense_pillars(dev):
    r = np.random.default_rng(7)
    a = synth.cloud_ring(2002)
    a = a[r.permutation(len(a))]                       # training-mode shuffle
    b = synth.cloud_uniform(1002, n=5000)
    b[:, :2] = b[:, :2] * 0.02 + np.array([10.0, 0.0], np.float32)   # ~100 pts per pillar: exercises P cap
    _check_voxel_parity([a, b], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4, dev)
    _check_voxel_parity([b], synth.PP_VOXEL, synth.PP_RANGE, 1, 50, 4, dev)      # P == 1, tiny cap


def test_voxelize_second_and_nuscenes_shapes(dev):
    frames = [synth.cloud_ring(2000), synth.cloud_uniform(1000, pc_range=synth.SEC_RANGE)]
    _check_voxel_parity(frames, synth.SEC_VOXEL, synth.SEC_RANGE, 5, 16000, 4, dev, repeat=1)
    _check_voxel_parity([synth.cloud_nus(4000), synth.cloud_nus(4001)[:12345]], synth.NUS_VOXEL, synth.NUS_RANGE, 10,
                        60000, 5, dev, repeat=1)


def test_voxelize_out_of_range_and_edges(dev):
    lo, hi = np.array(synth.PP_RANGE[:3], np.float32), np.array(synth.PP_RANGE[3:], np.float32)
    pts = np.array([[lo[0], lo[1], lo[2], 0.1], [hi[0], 0, 0, 0.2], [np.nextafter(hi[0], -np.inf, dtype=np.float32), 0, 0, 0.3],
                    [-0.001, 0, 0, 0.4], [5, 5, 1.0, 0.5], [5, 5, 0.999, 0.6], [5, 5, -3.0001, 0.7],
                    [0.16, 0.16, 0, 0.8], [0.15999, 0.16, 0, 0.9], [np.nan, 0, 0, 1.0], [1e9, 0, 0, 1.0]], np.float32)
    _check_voxel_parity([pts], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4, dev)


@pytest.mark.parametrize("algo", [0])
def test_voxelize_bin_overflow_falls_back(dev, algo):
    """20 000 points in ONE pillar put more entries into a single LDS hash bin than its entry list holds.  The LDS path
    (algo 0 -> 3) switches that bin to its streaming variant and stays exact WITHOUT raising the flag."""
    r = np.random.default_rng(3)
    pts = np.concatenate([r.uniform(10.0, 10.15, (20000, 2)), r.uniform(-2, 0, (20000, 1)), r.uniform(0, 1, (20000, 1))], 1).astype(np.float32)
    other = synth.cloud_ring(2003)[:3000]
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, algo=algo)
    exp = [c_oracle.voxelize(f, synth.PP_VOXEL, synth.PP_RANGE, 32, 16000) for f in (pts, other)]
    ev, ec, en = pp_oracle.collate(exp)
    for _ in range(2):
        out = vz.voxelize_frames([pts, other], device=dev)
        assert np.array_equal(out["voxel_coords"].cpu().numpy(), ec.astype(np.int32))
        assert np.array_equal(out["voxel_num_points"].cpu().numpy(), en)
        assert np.array_equal(out["voxels"].cpu().numpy(), ev)
        if algo == 0:
            assert vz.error_flag(2, 20000, dev) == 0
    out = vz.voxelize_frames([other], device=dev)      # and the fast path works again afterwards
    assert np.array_equal(out["voxels"].cpu().numpy(), exp[1][0])


def _zero_padded(frame, n_pad):
    return np.concatenate([frame, np.zeros((n_pad, frame.shape[1]), np.float32)], 0)


def test_voxelize_zero_padded_clouds_on_the_hot_path(dev):
    """Zero-padded frames (the padding lands in ONE voxel: (0,0,0) lies inside the KITTI range) through BatchVoxelizer.__call__
    — the sync-free entry the model forwards and bench.py use: exact, and no error flag (this used to drop points
    silently once a bin held more than 6144 entries)."""
    P, maxv = 32, 16000
    frames = [_zero_padded(synth.cloud_ring(2000)[:9000], 11000), _zero_padded(synth.cloud_uniform(1000, n=12000), 8000),
              synth.cloud_uniform(1001)]
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, P, maxv, 4)
    sizes = [len(f) for f in frames]
    pts = torch.from_numpy(np.concatenate(frames)).to(dev)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    for _ in range(2):
        o = vz(pts, offs, max(sizes), compact=True)
        offsets = o["voxel_offsets"].cpu().numpy()
        for f, pf in enumerate(frames):
            vo, co, nu = c_oracle.voxelize(pf, synth.PP_VOXEL, synth.PP_RANGE, P, maxv)
            a, b = int(offsets[f]), int(offsets[f + 1])
            assert b - a == len(vo), f
            assert np.array_equal(o["voxels"][a:b].cpu().numpy(), vo), f
            assert np.array_equal(o["voxel_num_points"][a:b].cpu().numpy(), nu)
            assert np.array_equal(o["voxel_coords"][a:b, 1:].cpu().numpy(), co)
    torch.cuda.synchronize()
    vz.poll_error()                                     # nothing was raised
    assert vz.error_flag(len(frames), max(sizes), dev) == 0


def test_voxelize_deadline_fallback_every_bin_workgroup(dev, monkeypatch):
    """csrc/voxelize.hip phase A1: a wave whose shared keys have not arrived by its deadline sets s_slow and the workgroup rebuilds
    its bin from the points themselves (vxl_bin_streaming).  An ordinary run never gets there, so the same source is built a second
    time with -DVXL_WAIT_TICKS=0 (csrc/build.py VARIANTS["vxl_nowait"]): EVERY bin workgroup of that library takes the deadline
    exit.  Same contract: bit-exact against the sequential oracle (data_processor.py:48-80 semantics), error flag 0 — on the
    PointPillar / SECOND / NuScenes shapes, a > 20 480-point frame (two key rounds), the zero-padded batch, through both entries
    (device offsets and host offsets) and in resident mode."""
    from lidardetection_amd import _lib
    from lidardetection_amd.csrc import build as hip_build
    variant = _lib.load_variant(hip_build.variant_path("vxl_nowait"))
    _lib.lib()
    monkeypatch.setattr(_lib, "_lib", variant)
    big = np.concatenate([synth.cloud_uniform(1003), synth.cloud_uniform(1004, n=9000)], 0)          # 29 000 points: two rounds
    cases = [([synth.cloud_ring(2000), synth.cloud_uniform(1000), np.zeros((0, 4), np.float32), synth.cloud_uniform(1001, n=333)],
              synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4),
             ([big, synth.cloud_ring(2001)[:7777]], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4),
             ([synth.cloud_ring(2000), synth.cloud_uniform(1000, pc_range=synth.SEC_RANGE)], synth.SEC_VOXEL, synth.SEC_RANGE, 5, 16000, 4),
             ([synth.cloud_nus(4000), synth.cloud_nus(4001)[:12345]], synth.NUS_VOXEL, synth.NUS_RANGE, 10, 60000, 5),
             ([_zero_padded(synth.cloud_ring(2000)[:9000], 11000), _zero_padded(synth.cloud_uniform(1000, n=12000), 8000),
               synth.cloud_uniform(1001)], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4)]
    for frames, vs, rng, P, maxv, C in cases:
        exp = [c_oracle.voxelize(f, vs, rng, P, maxv) for f in frames]
        ev, ec, en = pp_oracle.collate(exp)
        _check_one_algo(frames, vs, rng, P, maxv, C, dev, 2, 3, exp, ev, ec, en)
        sizes = [len(f) for f in frames]
        hoffs = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
        pts = torch.from_numpy(np.concatenate(frames)).to(dev)
        offs = torch.tensor(hoffs, dtype=torch.int32, device=dev)
        vz = BatchVoxelizer(vs, rng, P, maxv, C)
        out = vz.alloc_outputs(len(frames), dev)
        out["voxels"].fill_(float("nan"))
        for k in range(3):                              # resident mode + host offsets: first call full fill, then slot clears
            o = vz(pts, offs, max(sizes), out=out, resident=True, host_offsets=hoffs if k else None)
            total = int(o["voxel_offsets"][-1].item())
            assert total == len(ev)
            assert np.array_equal(o["voxels"][:total].cpu().numpy().view(np.uint32), ev.view(np.uint32))
            assert np.array_equal(o["voxel_coords"][:total].cpu().numpy(), ec.astype(np.int32))
            assert np.array_equal(o["voxel_num_points"][:total].cpu().numpy(), en)
            assert not o["voxels"][total:].any()
        assert vz.error_flag(len(frames), max(sizes), dev) == 0
        vz.poll_error()


def test_voxelize_refuses_bad_host_offsets(dev):
    """the LDS-binned launches read the points through the HOST offsets (kernel arguments); a stale list — another
    batch's, or one that ends beyond the point buffer — must be refused on the host before any launch."""
    from lidardetection_amd import _lib
    frames = [synth.cloud_uniform(1000, n=5000), synth.cloud_uniform(1001, n=4000)]
    pts = torch.from_numpy(np.concatenate(frames)).to(dev)
    offs = torch.tensor([0, 5000, 9000], dtype=torch.int32, device=dev)
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4)
    good = vz(pts, offs, 5000, host_offsets=[0, 5000, 9000])
    for bad in ([0, 5000, 9001], [0, 6000, 5000], [-1, 5000, 9000], [0, 5000], [0, 1, 9000], [0, 8000, 9000]):
        with pytest.raises(_lib.LidarHipError):
            vz(pts, offs, 5000, host_offsets=bad)
    again = vz(pts, offs, 5000, host_offsets=np.array([0, 5000, 9000]))
    assert torch.equal(good["voxels"][:int(good["voxel_offsets"][-1])], again["voxels"][:int(again["voxel_offsets"][-1])])


def _cells_of_one_bin(n_cells, G, nx=432, ny=496):
    """pillar centres of `n_cells` distinct PointPillar cells whose keys all fall into hash bin 0 of G (csrc/voxelize.hip)"""
    cell = np.arange(nx * ny, dtype=np.uint64)          # vxl_bin_of24: top log2(G) bits of a 24-bit multiplicative hash of the
    h = ((cell & np.uint64(0xFFFFFF)) * np.uint64(0x5BCA6B)) & np.uint64(0xFFFFFFFF)   # pillar cy * nx + cx (low 24 bits of the key)
    sel = cell[(h >> np.uint64(32 - int(np.log2(G)))) == 0][:n_cells].astype(np.int64)
    assert len(sel) == n_cells
    pts = np.zeros((n_cells, 4), np.float32)
    pts[:, 0] = (sel % nx + 0.5) * 0.16
    pts[:, 1] = (sel // nx + 0.5) * 0.16 - 39.68
    pts[:, 2] = -1.0
    return pts


def test_voxelize_true_bin_overflow_is_reported_without_a_sync(dev):
    """9 000 DISTINCT pillars in one LDS hash bin (adversarial: built from the hash itself) exceed the bin's 4 096-slot table.  The
    kernels mirror the sticky flag into pinned host memory: __call__ raises at the next call without any device read;
    voxelize_frames redoes the batch on the global-hash path and is exact."""
    from lidardetection_amd import _lib
    adv = _cells_of_one_bin(9000, G=16)                 # n_max 20000 -> 16 bins per frame (VXL_PTS_PER_BIN 1280)
    frames = [np.concatenate([adv, synth.cloud_uniform(1000, n=11000)], 0)]
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4)
    pts = torch.from_numpy(frames[0]).to(dev)
    offs = torch.tensor([0, len(frames[0])], dtype=torch.int32, device=dev)
    vz(pts, offs, 20000)
    torch.cuda.synchronize()                            # (only so that the test is deterministic: the mirror write has landed)
    with pytest.raises(_lib.LidarHipError):
        vz(pts, offs, 20000)
    out = vz.voxelize_frames(frames, device=dev)        # detects, falls back, exact
    vo, co, nu = c_oracle.voxelize(frames[0], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)
    assert np.array_equal(out["voxels"].cpu().numpy(), vo)
    assert np.array_equal(out["voxel_coords"][:, 1:].cpu().numpy(), co)
    assert np.array_equal(out["voxel_num_points"].cpu().numpy(), nu)


def test_pillar_vfe_vs_reference_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "pp_modules.npz"))
    t = lambda k, dt=None: torch.from_numpy(g[k]).to(dev) if dt is None else torch.from_numpy(g[k]).to(dev).to(dt)
    scale, shift = pillar_ops.fold_bn(t("bn_gamma"), t("bn_beta"), t("bn_mean"), t("bn_var"), float(g["bn_eps"]))
    vs, rng = [float(x) for x in g["voxel_size"]], [float(x) for x in g["pc_range"]]
    for cdt in (torch.int32, torch.float32):   # reference hands coords/counts over as float32
        out = pillar_ops.pillar_vfe(t("voxels"), t("num_points", cdt), t("coords", cdt), t("pfn_weight"), scale, shift, vs, rng)
        np.testing.assert_allclose(out.cpu().numpy(), g["pillar_features"], rtol=0, atol=1e-4)
        assert np.abs(out.cpu().numpy() - g["pillar_features"]).max() < 2e-5   # observed headroom
    mv = pillar_ops.mean_vfe(t("voxels"), t("num_points"))
    np.testing.assert_allclose(mv.cpu().numpy(), g["mean_features"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("P,C,V,with_distance", [(32, 4, 1001, False), (20, 4, 77, True), (40, 5, 333, False), (32, 5, 1, True), (64, 4, 129, False)])
def test_pillar_vfe_kernels_vs_oracle(dev, P, C, V, with_distance):
    """both PFN kernels — two voxels per wave iteration (P <= 32) and one (P <= 64) — against the torch-CPU restatement of
    PillarVFE / PFNLayer (oracle/pp_oracle.py, pinned by the reference golden above): odd voxel counts (a half-empty last pair),
    full and single-point pillars, 5 point features, with_distance, a device-side voxel count smaller than the buffer; 1e-4."""
    r = np.random.default_rng(P * 100 + C)
    num = r.integers(1, P + 1, V).astype(np.int32)
    num[:3] = [1, P, 2][:min(3, V)]
    vox = np.zeros((V, P, C), np.float32)
    coords = np.stack([r.integers(0, 2, V), np.zeros(V, np.int64), r.integers(0, 496, V), r.integers(0, 432, V)], 1).astype(np.int32)
    for v in range(V):
        ctr = np.array([coords[v, 3] * 0.16 + 0.08, coords[v, 2] * 0.16 - 39.6, -1.0] + [0.5] * (C - 3), np.float32)
        vox[v, :num[v]] = ctr + r.normal(0, 0.05, (num[v], C)).astype(np.float32)
    nf = C + 6 + int(with_distance)
    w = (r.standard_normal((64, nf)) * 0.3).astype(np.float32)
    gamma, beta = r.uniform(0.5, 1.5, 64).astype(np.float32), (r.standard_normal(64) * 0.2).astype(np.float32)
    mean, var = (r.standard_normal(64) * 0.1).astype(np.float32), r.uniform(0.5, 1.5, 64).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    scale, shift = pillar_ops.fold_bn(t(gamma), t(beta), t(mean), t(var), 1e-3)
    pad = 5                                                               # rows past the device-side count must be ignored
    voxd = torch.cat([t(vox), torch.full((pad, P, C), 7.0, device=dev)], 0)
    numd = torch.cat([t(num), torch.full((pad,), P, dtype=torch.int32, device=dev)], 0)
    cd = torch.cat([t(coords), torch.zeros((pad, 4), dtype=torch.int32, device=dev)], 0)
    out = pillar_ops.pillar_vfe(voxd, numd, cd, t(w), scale, shift, synth.PP_VOXEL, synth.PP_RANGE, with_distance=with_distance,
                                num_voxels_dev=torch.tensor([V], dtype=torch.int32, device=dev))
    ref = pp_oracle.pillar_vfe(torch.from_numpy(vox), torch.from_numpy(num).float(), torch.from_numpy(coords).float(), torch.from_numpy(w),
                               torch.from_numpy(gamma), torch.from_numpy(beta), torch.from_numpy(mean), torch.from_numpy(var),
                               synth.PP_VOXEL, synth.PP_RANGE, eps=1e-3, with_distance=with_distance)
    np.testing.assert_allclose(out[:V].cpu().numpy(), ref.numpy(), rtol=0, atol=1e-4)


def test_pillar_scatter_vs_reference_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "pp_modules.npz"))
    shp = tuple(int(x) for x in g["canvas_shape"])
    ref = np.zeros(shp, np.float32)
    ref[tuple(g["canvas_nz_idx"])] = g["canvas_nz_val"]
    feat = torch.from_numpy(g["pillar_features"]).to(dev)
    for cdt in (torch.int32, torch.float32):
        canvas = pillar_ops.pillar_scatter(feat, torch.from_numpy(g["coords"]).to(dev).to(cdt), shp[0], shp[3], shp[2])
        assert np.array_equal(canvas.cpu().numpy(), ref)


def test_pillar_scatter_full_kitti_grid(dev):
    """PointPillar-KITTI canvas 64 x 496 x 432, bs=2, against the oracle scatter."""
    frames = [synth.cloud_ring(2000), synth.cloud_uniform(1000)]
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)
    o = vz.voxelize_frames(frames, device=dev)
    V = o["voxels"].shape[0]
    feat = torch.randn(V, 64, device=dev)
    canvas = pillar_ops.pillar_scatter(feat, o["voxel_coords"], 2, 432, 496)
    exp = pp_oracle.pillar_scatter(feat.cpu(), o["voxel_coords"].cpu().float(), 2, 432, 496)
    assert torch.equal(canvas.cpu(), exp)
    nhwc = pillar_ops.pillar_scatter(feat, o["voxel_coords"], 2, 432, 496, channels_last=True)   # same tensor, NHWC strides
    assert nhwc.is_contiguous(memory_format=torch.channels_last) and torch.equal(nhwc.cpu(), exp)


def test_iou_matrices_vs_reference_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "iou3d_ref.npz"))
    a, b = torch.from_numpy(g["boxes_a"]).to(dev), torch.from_numpy(g["boxes_b"]).to(dev)
    iou = iou3d_nms_utils.boxes_iou_bev(a, b).cpu().numpy()
    # device trig / atan2 differ from glibc by ulps: 1e-5 absolute on IoU in [0,1] (north_star: 1e-4)
    np.testing.assert_allclose(iou, g["iou_bev_cpu"], rtol=0, atol=1e-5)
    assert np.array_equal(iou == 0, g["iou_bev_cpu"] == 0)     # the exact-zero early-out agrees
    ov = torch.zeros(len(a), len(b), device=dev)
    iou3d_nms_cuda.boxes_overlap_bev_gpu(a, b, ov)
    np.testing.assert_allclose(ov.cpu().numpy(), c_oracle.pairwise(g["boxes_a"], g["boxes_b"], 0), rtol=1e-5, atol=1e-5)
    # boxes_iou3d_gpu (iou3d_nms_utils.py:48-81): BEV overlap x height overlap / union volume
    i3 = iou3d_nms_utils.boxes_iou3d_gpu(a, b).cpu().numpy()
    A, B = g["boxes_a"], g["boxes_b"]
    ovo = c_oracle.pairwise(A, B, 0)
    h = np.clip(np.minimum((A[:, 2] + A[:, 5] / 2)[:, None], (B[:, 2] + B[:, 5] / 2)[None]) -
                np.maximum((A[:, 2] - A[:, 5] / 2)[:, None], (B[:, 2] - B[:, 5] / 2)[None]), 0, None)
    o3 = ovo * h
    va, vb = (A[:, 3] * A[:, 4] * A[:, 5])[:, None], (B[:, 3] * B[:, 4] * B[:, 5])[None]
    np.testing.assert_allclose(i3, o3 / np.clip(va + vb - o3, 1e-6, None), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("thresh", [0.01, 0.1, 0.7])
@pytest.mark.parametrize("seed,objects", [(3000, 512), (3001, 100), (3002, 33), (3003, 530)])  # 530*8 > 4096: slow-path greedy
def test_rotated_nms_keep_bit_exact(dev, thresh, seed, objects):
    boxes, scores = synth.boxes_nms(seed=seed, objects=objects, copies=8)
    if objects == 33:
        boxes, scores = boxes[:-3], scores[:-3]      # N not a multiple of 64
    order = np.argsort(-scores, kind="stable")
    bs = boxes[order]
    mask_o = c_oracle.nms_mask(bs, thresh)
    keep_o = c_oracle.nms_greedy(mask_o)
    # pairs whose oracle IoU sits within 2e-6 of the threshold could legitimately flip with the ulp-level
    # differences between glibc and the device's trig/atan2; they are counted and reported, and the
    # fixtures are seeded so that the decisions still agree bit for bit (asserted below).
    iou = c_oracle.pairwise(bs, bs, 1)
    near = int((np.abs(iou[iou > 0] - thresh) < 2e-6).sum())
    print(f"pairs within 2e-6 of thresh {thresh}: {near} of {(iou > 0).sum()}")
    tb = torch.from_numpy(bs).to(dev)
    mask_d = iou3d_nms_cuda.nms_mask_debug(tb, thresh).cpu().numpy().view(np.uint64)
    n, cb = mask_o.shape
    for i in range(n):   # compare the upper-triangular words the greedy reads
        assert np.array_equal(mask_d[i, i // 64:], mask_o[i, i // 64:]), f"mask row {i}"
    keep = torch.LongTensor(n)
    num = iou3d_nms_cuda.nms_gpu(tb, keep, thresh)
    assert keep[:num].tolist() == keep_o.tolist()
    sel, _ = iou3d_nms_utils.nms_gpu(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), thresh)
    assert sel.cpu().tolist() == order[keep_o].tolist()


@pytest.mark.parametrize("thresh", [0.01, 0.1, 0.7])
@pytest.mark.parametrize("seed,objects,copies", [(3020, 2, 700), (3021, 3, 500)])
def test_rotated_nms_dense_tiles_bit_exact(dev, thresh, seed, objects, copies):
    """A few objects with hundreds of proposals each: almost every pair of a 64x64 tile passes the bounding-circle test, so the
    tile has more candidates than the pair list holds (NMS_PAIR_CAP) and runs in four 16-row rounds (this path
    had no test).  Mask words and keep list vs the oracle; pairs whose oracle IoU lies within 2e-6 of the threshold may flip
    with the last ulp of the trig functions and are taken from the device before the greedy replay."""
    boxes, scores = synth.boxes_nms(seed=seed, objects=objects, copies=copies)
    order = np.argsort(-scores, kind="stable")
    bs = boxes[order]
    n = len(bs)
    mask_o = c_oracle.nms_mask(bs, thresh)
    iou = c_oracle.pairwise(bs, bs, 1)
    assert ((iou > 0).sum() - n) / (n * (n - 1)) > 0.25          # dense: over a quarter of all pairs overlap
    tb = torch.from_numpy(bs).to(dev)
    mask_d = iou3d_nms_cuda.nms_mask_debug(tb, thresh).cpu().numpy().view(np.uint64)
    near = np.argwhere(np.abs(iou - thresh) < 2e-6)
    assert len(near) <= 1e-5 * n * (n - 1), f"{len(near)} of {n * (n - 1)} ordered pairs patched: the escape hatch is bounded at 1e-5"
    for i, j in near:
        if j > i:                                                  # upper triangle only (what the greedy reads)
            bit = np.uint64(1) << np.uint64(j % 64)
            mask_o[i, j // 64] = (mask_o[i, j // 64] & ~bit) | (mask_d[i, j // 64] & bit)
    print(f"thr {thresh}: {len(near)} pairs within 2e-6 of the threshold")
    for i in range(n):
        assert np.array_equal(mask_d[i, i // 64:], mask_o[i, i // 64:]), f"mask row {i}"
    keep_o = c_oracle.nms_greedy(mask_o)
    keep = torch.LongTensor(n)
    num = iou3d_nms_cuda.nms_gpu(tb, keep, thresh)
    assert keep[:num].tolist() == keep_o.tolist()


@pytest.mark.parametrize("seed,thresh", [(3020, 0.1), (3034, 0.01), (3034, 0.1), (3035, 0.01), (3035, 0.1)])
def test_rotated_nms_dense_tiles_bit_exact_without_patching(dev, seed, thresh):
    """Dense-tile fixtures (2 objects x 700 proposals, half of all pairs overlap) in which NO pair lies within 2e-6 of the
    threshold (asserted from the oracle's IoU matrix): device mask words and keep list vs the oracle with nothing patched."""
    boxes, scores = synth.boxes_nms(seed=seed, objects=2, copies=700)
    bs = boxes[np.argsort(-scores, kind="stable")]
    n = len(bs)
    iou = c_oracle.pairwise(bs, bs, 1)
    assert int((np.abs(iou - thresh) < 2e-6).sum()) == 0 and ((iou > 0).sum() - n) / (n * (n - 1)) > 0.25
    mask_o = c_oracle.nms_mask(bs, thresh)
    tb = torch.from_numpy(bs).to(dev)
    mask_d = iou3d_nms_cuda.nms_mask_debug(tb, thresh).cpu().numpy().view(np.uint64)
    for i in range(n):
        assert np.array_equal(mask_d[i, i // 64:], mask_o[i, i // 64:]), f"mask row {i}"
    keep = torch.LongTensor(n)
    num = iou3d_nms_cuda.nms_gpu(tb, keep, thresh)
    assert keep[:num].tolist() == c_oracle.nms_greedy(mask_o).tolist()


def test_nms_normal_and_pre_maxsize(dev):
    boxes, scores = synth.boxes_nms(seed=3005, objects=128, copies=8)
    tb, ts = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    sel, _ = iou3d_nms_utils.nms_normal_gpu(tb, ts, 0.3)
    assert sel.cpu().tolist() == c_oracle.nms(boxes, scores, 0.3, normal=True).tolist()
    sel, _ = iou3d_nms_utils.nms_gpu(tb, ts, 0.1, pre_maxsize=300)
    assert sel.cpu().tolist() == c_oracle.nms(boxes, scores, 0.1, pre_maxsize=300).tolist()
    # empty and single-box inputs
    e, _ = iou3d_nms_utils.nms_gpu(tb[:0], ts[:0], 0.1)
    assert e.numel() == 0
    o, _ = iou3d_nms_utils.nms_gpu(tb[:1], ts[:1], 0.1)
    assert o.cpu().tolist() == [0]


def test_nms_batched_counts(dev):
    """Batched device-resident NMS with ragged per-frame counts == per-frame oracle."""
    sets = [synth.boxes_nms(seed=3010 + k, objects=40 + 17 * k, copies=8) for k in range(4)]
    nmax = max(len(b) for b, _ in sets)
    bt = torch.zeros(4, nmax, 7)
    cnt = []
    exp = []
    for k, (b, s) in enumerate(sets):
        o = np.argsort(-s, kind="stable")
        bt[k, :len(b)] = torch.from_numpy(b[o])
        cnt.append(len(b))
        exp.append(c_oracle.nms_sorted(b[o], 0.1))
    keep, num = iou3d_nms_cuda.nms_batch(bt.to(dev), torch.tensor(cnt, dtype=torch.int32, device=dev), 0.1)
    for k in range(4):
        assert keep[k, :int(num[k])].cpu().tolist() == exp[k].tolist()


# ------------------------------------------------------------------ dense BEV backbone epilogue
@pytest.mark.parametrize("shape,cout,off,relu", [((2, 64, 31, 17), 64, 0, True), ((3, 128, 8, 12), 384, 128, True),
                                                 ((1, 72, 5, 7), 72, 0, False)])
def test_bias_act_nhwc_bit_exact(dev, shape, cout, off, relu):
    from lidardetection_amd.bev_backbone import bias_act_
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    b = torch.randn(shape[1], generator=g).to(dev)
    want = x + b.view(1, -1, 1, 1)
    want = torch.relu(want) if relu else want
    if cout == shape[1]:
        got = bias_act_(x.clone(memory_format=torch.channels_last), b, relu=relu)
        assert torch.equal(got, want)
    else:
        out = torch.full((shape[0], cout, shape[2], shape[3]), -7.0, device=dev).contiguous(memory_format=torch.channels_last)
        bias_act_(x, b, relu=relu, out=out, out_offset=off)
        assert torch.equal(out[:, off:off + shape[1]], want)
        rest = torch.cat([out[:, :off], out[:, off + shape[1]:]], 1)
        assert torch.all(rest == -7.0)          # neighbouring channel slices untouched


def test_folded_bev_backbone_matches_stock_modules(dev):
    """BN folded into the convs + one-pass HIP epilogue + merged heads vs the unfolded torch modules (fp32, 1e-4)."""
    from lidardetection_amd.pointpillar import PointPillarKITTI
    m = PointPillarKITTI(batch_size=2, device=dev).randomize_for_bench(3)
    assert m.fold_bn
    g = torch.Generator(device="cpu").manual_seed(11)
    canvas = torch.randn(2, 64, m.ny, m.nx, generator=g).to(dev)
    canvas[:, :, ::3] = 0
    canvas = canvas.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = m.split_heads(m.backbone_head(canvas)[0])
        want = m.backbone_head_stock(canvas)
    for a, b, name in zip(got, want, ("cls", "box", "dir")):
        assert a.shape == b.shape, name
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-4 * max(scale, 1.0), name


@pytest.mark.parametrize("s", [1, 2, 4])
def test_deblock_as_gemm_with_pixel_shuffle_epilogue(dev, s):
    """ConvTranspose2d(kernel == stride) = GEMM + shuffle epilogue, vs torch's conv_transpose2d (fp32, 1e-5)."""
    from lidardetection_amd.bev_backbone import bias_act_upsample_
    g = torch.Generator(device="cpu").manual_seed(5 + s)
    B, Cin, Cout, h, w = 2, 24, 16, 7, 9
    x = torch.randn(B, Cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(Cin, Cout, s, s, generator=g) * 0.2).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    want = torch.relu(torch.nn.functional.conv_transpose2d(x, wt, b, stride=s))
    out = torch.full((B, 40, h * s, w * s), -3.0, device=dev).contiguous(memory_format=torch.channels_last)
    y = torch.mm(x.permute(0, 2, 3, 1).reshape(B * h * w, Cin), wt.permute(0, 2, 3, 1).reshape(Cin, -1).contiguous())
    bias_act_upsample_(y, b, B, h, w, s, out, 8)
    np.testing.assert_allclose(out[:, 8:24].cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5)
    assert torch.all(out[:, :8] == -3.0) and torch.all(out[:, 24:] == -3.0)


def test_fused_anchor_post_processing_matches_torch_ops(dev):
    """HIP score / top-k decode kernels on the merged head output vs the reference's op sequence in torch (sigmoid, max,
    threshold mask, topk, ResidualCoder.decode_torch, direction bins): scores, labels and boxes bit-exact, NMS output equal."""
    from lidardetection_amd import anchor_post
    from lidardetection_amd.pointpillar import PointPillarKITTI
    m = PointPillarKITTI(batch_size=2, device=dev).randomize_for_bench(5)
    g = torch.Generator(device="cpu").manual_seed(17)
    H, W, a = m.ny // 2, m.nx // 2, m.num_anchor_per_loc
    head = torch.randn(2, H, W, a * (m.num_class + 7 + m.num_dir_bins), generator=g)
    head[..., :a * m.num_class] *= 3.0                                   # spread the class logits across the threshold
    head[..., a * m.num_class:a * (m.num_class + 7)] *= 0.3
    head = head.to(dev)
    cls, box, dirs = m.split_heads(head)
    with torch.no_grad():
        scores_all, labels_all = torch.sigmoid(cls).max(dim=-1)
        want_masked = torch.where(scores_all >= m.score_thresh, scores_all, scores_all.new_full((), -1.0))
        got_masked, got_labels = anchor_post.anchor_scores(head, a, m.num_class, m.score_thresh)
        assert torch.equal(got_masked, want_masked)
        assert torch.equal(got_labels.long(), labels_all)
        k = 4096
        top_scores, top_idx = torch.topk(want_masked, k, dim=1)
        gi = top_idx.unsqueeze(-1)
        want_boxes = m.decode(torch.gather(box, 1, gi.expand(-1, -1, 7)), m.anchors[top_idx],
                              torch.gather(dirs, 1, gi.expand(-1, -1, m.num_dir_bins)))
        got_boxes = anchor_post.decode_topk(head, top_idx, m.anchors, a, a * m.num_class, a * (m.num_class + 7),
                                            m.num_dir_bins, m.dir_offset, m.dir_limit_offset)
        assert torch.equal(got_boxes, want_boxes)
        # the HIP top-k (scores + histogram, collect, finalize) selects what torch.topk selects — and in the same order where
        # scores are distinct; among equal scores the lower anchor index comes first (torch leaves that unspecified)
        ws = anchor_post.topk_workspace(2, want_masked.shape[1], dev)
        m2, l2 = anchor_post.anchor_scores(head, a, m.num_class, m.score_thresh, topk_ws=ws)
        assert torch.equal(m2, want_masked) and torch.equal(l2, got_labels)
        hs, hi, hc = anchor_post.topk_desc(m2, k, m.score_thresh, ws, hist_ready=True)
        ts_o, ti_o, cnt_o = _topk_reference(want_masked.cpu().numpy(), k, m.score_thresh)
        assert np.array_equal(hs.cpu().numpy(), ts_o) and np.array_equal(hi.cpu().numpy(), ti_o) and np.array_equal(hc.cpu().numpy(), cnt_o)
        assert torch.equal(hs, top_scores)
        distinct = torch.ones_like(top_scores, dtype=torch.bool)
        distinct[:, 1:] &= top_scores[:, 1:] != top_scores[:, :-1]
        distinct[:, :-1] &= top_scores[:, 1:] != top_scores[:, :-1]
        assert torch.equal(hi[distinct], top_idx[distinct])
        fused = m.post_process(head)
    # final detections: the reference's op sequence on the HIP selection (ties resolved by index)
    with torch.no_grad():
        gi2 = hi.unsqueeze(-1)
        boxes2 = m.decode(torch.gather(box, 1, gi2.expand(-1, -1, 7)), m.anchors[hi], torch.gather(dirs, 1, gi2.expand(-1, -1, m.num_dir_bins))).contiguous()
        plain = m._nms_and_gather(boxes2, hs, hi, labels_all, hc, k)
    for x, y in zip(fused, plain):
        assert torch.equal(x, y)


def _topk_reference(scores, k, valid_min):
    """(score desc, index asc) over the scores >= valid_min; slots past the valid count are (-1, 0)"""
    B, n = scores.shape
    ts, ti, cnt = np.full((B, k), -1.0, np.float32), np.zeros((B, k), np.int64), np.zeros(B, np.int32)
    for b in range(B):
        valid = np.nonzero(scores[b] >= np.float32(valid_min))[0]
        order = valid[np.lexsort((valid, -scores[b][valid].astype(np.float64)))][:k]
        ts[b, :len(order)], ti[b, :len(order)], cnt[b] = scores[b][order], order, len(order)
    return ts, ti, cnt


@pytest.mark.parametrize("case", ["distinct", "quantised", "tie_mass", "tie_mass_plus", "few_valid", "none_valid", "big_bin_distinct", "small_k"])
def test_topk_desc_exact_deterministic_with_ties(dev, case):
    """lidar_topk_desc (csrc/topk.hip) against a stable CPU sort: descending score, ties by ascending index — the rule is
    checked on tens of thousands of bit-equal scores (empty BEV regions), on a bin of > 8 192 DISTINCT keys around the k-th score
    (the radix-select path), with fewer valid scores than k, with none, and for k < 4096; torch.topk agrees wherever scores are
    distinct."""
    from lidardetection_amd import anchor_post
    r = np.random.default_rng(__import__("zlib").crc32(case.encode()) % 1000)   # fixed per case: hash() changes with PYTHONHASHSEED
    B, n, k, thr = 3, 321408, 4096, 0.1
    s = r.uniform(0.0, 1.0, (B, n)).astype(np.float32)
    if case == "quantised":
        s = (np.round(s * 200) / 200).astype(np.float32)                       # ~1 600 equal scores per level
    elif case == "tie_mass":
        s[:] = np.float32(0.3)                                                  # every score equal
    elif case == "tie_mass_plus":
        s = np.where(r.uniform(size=(B, n)) < 0.01, s * 0.5 + 0.5, np.float32(0.47)).astype(np.float32)   # 3 200 above one tie mass of 318 k
    elif case == "few_valid":
        s[:, 1000:] *= np.float32(0.05)                                         # 1 000 candidates, the rest below the threshold
    elif case == "none_valid":
        s *= np.float32(0.09)
    elif case == "big_bin_distinct":
        base = np.float32(0.5).view(np.uint32)
        d = (base + r.permutation(12000).astype(np.uint32)).view(np.float32)     # 12 000 distinct scores inside ONE histogram bin
        s[:] = np.float32(0.2) * s                                              # everything else far below (most under the threshold)
        for b in range(B):
            s[b, r.choice(n, 12000, replace=False)] = d
        s[:, :500] = np.float32(0.9) + np.float32(1e-4) * r.uniform(size=(B, 500)).astype(np.float32)   # and 500 clearly above
    elif case == "small_k":
        k = 1000
    s[s < thr] = -1.0                                                           # as anchor_scores masks them
    ts_o, ti_o, cnt_o = _topk_reference(s, k, thr)
    td = torch.from_numpy(s).to(dev)
    for _ in range(2):                                                          # twice: the workspace cleans up after itself
        ts, ti, cnt = anchor_post.topk_desc(td, k, thr)
        assert np.array_equal(cnt.cpu().numpy(), cnt_o), case
        assert np.array_equal(ts.cpu().numpy(), ts_o), case
        assert np.array_equal(ti.cpu().numpy(), ti_o), case
    if case == "distinct":
        tt, it = torch.topk(td, k, dim=1)
        assert torch.equal(tt, ts) and torch.equal(it, ti)


@pytest.mark.parametrize("case", ["logits_no_threshold", "negative_threshold", "zero_threshold", "all_negative_ties", "with_nan_and_inf"])
def test_topk_desc_signed_scores(dev, case):
    """r04: the selection key is an order-preserving map of the float bits, so lidar_topk_desc ranks scores of any sign — the raw class
    logits PV-RCNN's proposal layer ranks (pcdet/models/roi_heads/roi_head_template.py:45-99: no threshold) — against a stable CPU sort;
    slots past the count hold (-inf, 0) when the threshold is not positive.  For distinct scores torch.topk agrees."""
    from lidardetection_amd import anchor_post
    r = np.random.default_rng(__import__("zlib").crc32(case.encode()) % 1000)
    B, n, k = 2, 211200, 1024
    s = r.normal(-4.0, 2.0, (B, n)).astype(np.float32)
    thr, smax = -np.inf, float(np.finfo(np.float32).max)
    if case == "negative_threshold":
        thr, smax = -0.5, 20.0
    elif case == "zero_threshold":
        s = r.normal(0.0, 1.0, (B, n)).astype(np.float32)
        s[:, ::7] = 0.0
        s[:, 3::11] = -0.0                                                   # -0.0 >= 0.0 is true: a candidate, and it TIES with +0.0
        thr, smax = 0.0, 10.0
    elif case == "all_negative_ties":
        s = (np.round(s * 4) / 4).astype(np.float32)                            # quarter steps: thousands of equal negative scores
    elif case == "with_nan_and_inf":
        s[0, 5], s[0, 77], s[1, 9], s[1, 100] = np.nan, np.inf, -np.inf, np.nan
    td = torch.from_numpy(s).to(dev)
    ts, ti, cnt = anchor_post.topk_desc(td, k, thr, score_max=smax)
    for b in range(B):
        valid = np.nonzero(s[b] >= np.float32(thr))[0]                          # (NaN >= x is False: never a candidate)
        sv = s[b][valid]
        order = valid[np.lexsort((valid, -sv.astype(np.float64)))][:k]          # descending value, ties (incl. -0.0 / +0.0) by ascending index
        assert int(cnt[b]) == len(order), case
        got_i, got_s = ti[b, :len(order)].cpu().numpy(), ts[b, :len(order)].cpu().numpy()
        assert np.array_equal(got_s, s[b][order]), case                         # (value equality: a -0.0 comes back as +0.0)
        assert np.array_equal(got_i, order), case
        if len(order) < k:
            assert np.all(np.isneginf(ts[b, len(order):].cpu().numpy())) and not ti[b, len(order):].any()
    if case == "logits_no_threshold":
        tt, it = torch.topk(td, k, dim=1)
        assert torch.equal(tt, ts) and torch.equal(it, ti)


def test_nms_batch_max_keep_is_a_prefix_of_the_full_result(dev):
    """max_keep (NMS_POST_MAXSIZE) stops the greedy pass early: the survivors it reports are the first ones of the full run"""
    from lidardetection_amd.ext import iou3d_nms_cuda
    bt = []
    for k in range(3):
        b, s = synth.boxes_nms(seed=3100 + k)
        bt.append(torch.from_numpy(b[np.argsort(-s, kind="stable")]))
    boxes = torch.stack(bt).to(dev)
    counts = torch.tensor([4096, 3000, 70], dtype=torch.int32, device=dev)
    full_keep, full_num = iou3d_nms_cuda.nms_batch(boxes, counts, 0.1)
    for mk in (1, 64, 100, 500, 5000):
        keep, num = iou3d_nms_cuda.nms_batch(boxes, counts, 0.1, max_keep=mk)
        want = torch.clamp(full_num, max=mk)
        assert torch.equal(num, want)
        for f in range(3):
            assert torch.equal(keep[f, :int(want[f])], full_keep[f, :int(want[f])])


def test_nms_batch_limited_second_stage_frames(dev):
    """The limited call builds the mask of the first 2 max_keep candidates only and redoes, in full, just the frames that ran out of
    survivors there (csrc/iou3d.hip lidar_nms_batch_limited).  Frame 0: 60 tight clusters -> far fewer than max_keep survivors, the
    second stage must supply the complete answer; frame 1: spread boxes -> finished by the first stage; frame 2: clusters in the
    first 1 500 candidates, spread boxes after them -> the survivors straddle the first-stage limit."""
    from lidardetection_amd.ext import iou3d_nms_cuda
    r = np.random.default_rng(77)
    n = 4096

    def clustered(m, k):
        c = r.uniform(-60, 60, (k, 2)).astype(np.float32)
        idx = r.integers(0, k, m)
        b = np.zeros((m, 7), np.float32)
        b[:, :2] = c[idx] + r.normal(0, 0.05, (m, 2)).astype(np.float32)
        b[:, 3:6] = (3.9, 1.6, 1.5)
        b[:, 6] = r.uniform(-0.1, 0.1, m)
        return b

    def spread(m):
        b = np.zeros((m, 7), np.float32)
        b[:, :2] = r.uniform(-200, 200, (m, 2))
        b[:, 3:6] = (3.9, 1.6, 1.5)
        b[:, 6] = r.uniform(-3.1, 3.1, m)
        return b

    frames = [clustered(n, 60), spread(n), np.concatenate([clustered(1500, 40), spread(n - 1500)])]
    boxes = torch.from_numpy(np.stack(frames)).to(dev)
    counts = torch.tensor([n, n, 3900], dtype=torch.int32, device=dev)
    full_keep, full_num = iou3d_nms_cuda.nms_batch(boxes, counts, 0.1)
    assert int(full_num[0]) < 100 and int(full_num[1]) > 2000
    for mk in (100, 300, 500):
        keep, num = iou3d_nms_cuda.nms_batch(boxes, counts, 0.1, max_keep=mk)
        want = torch.clamp(full_num, max=mk)
        assert torch.equal(num, want), (mk, num, want)
        for f in range(3):
            assert torch.equal(keep[f, :int(want[f])], full_keep[f, :int(want[f])]), (mk, f)


def test_bev_backbone_and_box_decode_vs_reference_golden(dev, golden_dir):
    """tests/golden/bev_head.npz was emitted by the REFERENCE's own BaseBEVBackbone and ResidualCoder.decode_torch
    (tests/golden/make_golden.py).  The folded backbone (BN folded, HIP epilogues, GEMM deblocks writing the concat slice) must
    reproduce the reference module's output from the reference's own state_dict; lidar_decode_topk must reproduce its decode."""
    import torch.nn as nn
    from lidardetection_amd import anchor_post
    from lidardetection_amd.bev_backbone import FoldedBEVBackbone
    from lidardetection_amd.pointpillar import make_bev_backbone
    g = np.load(os.path.join(golden_dir, "bev_head.npz"))

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks, self.deblocks = make_bev_backbone(cin=16, layer_nums=(1, 2), strides=(2, 2), filters=(16, 32),
                                                           up_strides=(1, 2), up_filters=(32, 32))
    h = Holder()
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("bev.")}
    h.load_state_dict(sd, strict=True)                      # the reference's parameter names fit this repo's module tree
    h = h.to(dev).eval().to(memory_format=torch.channels_last)
    heads = [nn.Conv2d(64, 4, 1).to(dev)]
    x = torch.from_numpy(g["bev_input"]).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = FoldedBEVBackbone(h.blocks, h.deblocks, heads).features(x)
    want = g["bev_output"]
    assert tuple(got.shape) == want.shape
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    # ResidualCoder.decode_torch: one anchor per location, no direction bins
    enc, anchors = torch.from_numpy(g["decode_enc"]).to(dev), torch.from_numpy(g["decode_anchors"]).to(dev)
    n = enc.shape[0]
    boxes = anchor_post.decode_topk(enc.view(1, n, 7).contiguous(), torch.arange(n, device=dev).view(1, n), anchors, 1, box_off=0,
                                    dir_off=0, num_dir_bins=0, dir_offset=0.0, dir_limit_offset=0.0)
    np.testing.assert_allclose(boxes[0].cpu().numpy(), g["decode_out"], rtol=2e-6, atol=1e-6)


def _bev_wide_inputs(golden_dir, dev):
    """tests/golden/bev_wide.npz -> (fixture, module holder on `dev`, channels-last canvas, PillarMap of its occupied cells)"""
    import copy
    from test_oracle_pins import _bev_wide
    g, h = _bev_wide(golden_dir)
    h = copy.deepcopy(h).to(dev).to(memory_format=torch.channels_last)
    x = torch.from_numpy(g["bev_input"])
    B, C, H, W = x.shape
    b, yy, xx = (x.abs().sum(1) > 0).nonzero(as_tuple=True)
    perm = torch.randperm(len(b), generator=torch.Generator().manual_seed(5))       # pillars in no particular order
    b, yy, xx = b[perm], yy[perm], xx[perm]
    feats = x.permute(0, 2, 3, 1)[b, yy, xx].contiguous().to(dev)
    coords = torch.stack([b, torch.zeros_like(b), yy, xx], 1).to(torch.int32).to(dev)
    total = torch.tensor([len(b)], dtype=torch.int32, device=dev)
    pm = pillar_ops.PillarMap(feats, coords, total, B, W, H,
                              lambda f, c, n: pillar_ops.pillar_scatter(f, c, B, W, H, num_voxels_dev=n, channels_last=True))
    return g, h, x.to(dev).contiguous(memory_format=torch.channels_last), pm


def _wide_heads(dev, cin, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    heads = [torch.nn.Conv2d(cin, 18, 1), torch.nn.Conv2d(cin, 14, 1)]
    with torch.no_grad():
        for hd in heads:
            hd.weight.copy_(torch.randn(hd.weight.shape, generator=g) / cin ** 0.5)
            hd.bias.copy_(torch.randn(hd.bias.shape, generator=g) * 0.1)
    return [hd.to(dev).to(memory_format=torch.channels_last) for hd in heads]


def _heads_fp64(feat, heads):
    """fp64 1x1 convolutions of a (B, C, H, W) map -> (B, H, W, sum C_head) in the order merged() writes them"""
    wt = torch.cat([hd.weight.detach().double().cpu().flatten(1) for hd in heads], 0)
    b = torch.cat([hd.bias.detach().double().cpu() for hd in heads], 0)
    return torch.einsum("bchw,nc->bhwn", torch.as_tensor(feat).double(), wt) + b


class _Calls:
    """counts calls of module-level functions (monkeypatched attributes) -> which routes the folded backbone really took"""

    def __init__(self, monkeypatch, *targets):
        self.n = {}
        for mod, name in targets:
            fn = getattr(mod, name)
            self.n[name] = 0

            def wrapped(*a, _fn=fn, _name=name, **k):
                self.n[_name] += 1
                return _fn(*a, **k)
            monkeypatch.setattr(mod, name, wrapped)

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.n, 0)
        return out


def _check_folded_entries(bev, canvas, pm, want, want_head, tag, split):
    """features() from the canvas and from the sparse first layer, merged() from the canvas and from the pillars (as the two-stream
    split when `split`), against the fp64 feature map / head output: <= 1e-4 of scale.  -> the largest error of each (printed by -s)"""
    tol = 1e-4 * max(1.0, float(np.abs(want).max()))
    tol_h = 1e-4 * max(1.0, float(want_head.abs().max()))
    errs = {}
    with torch.no_grad():
        for name, run in (("features(canvas)", lambda: bev.features(canvas)),
                          ("features(sparse first)", lambda: bev.features(bev.first_layer_from_pillars(pm), first_done=True))):
            got = run()
            assert tuple(got.shape) == want.shape, (tag, name)
            errs[name] = float(np.abs(got.cpu().numpy() - want).max())
        for name, src in (("merged(canvas)", canvas), ("merged(pillars)", pm)):
            bev._streams = None
            got = bev.merged(src)
            assert tuple(got.shape) == tuple(want_head.shape), (tag, name)
            assert (bev._streams is not None) == split, (tag, name, "two-stream split taken / not taken")
            errs[name] = float((got.double().cpu() - want_head).abs().max())
    print(f"[bev_wide {tag}] " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f" (feature tol {tol:.1e}, head tol {tol_h:.1e})")
    for k, v in errs.items():
        assert v <= (tol_h if k.startswith("merged") else tol), (tag, k, v)
    return errs


def test_folded_bev_backbone_production_routes_vs_reference_golden(dev, golden_dir, monkeypatch):
    """tests/golden/bev_wide.npz: the reference's own BaseBEVBackbone in float64 on a configuration wide enough for the production
    routes (64 / 64 filters, 128 / 128 upsample filters).  FoldedBEVBackbone must take them — F(4x4, 3x3) Winograd for both
    stride-1 layers (block 1 runs on a 6 x 5 map: partial tiles at the edges), the fused deblock GEMM (csrc/deconv_gemm.hip) for the
    stride-2 deblock, the strided-epilogue hipBLASLt GEMM for the stride-1 deblock, the sparse first layer from the pillars — and
    reproduce the fixture through features() and merged(), from the canvas and from the pillars, whole-batch and as the two-stream
    split; then again with the byte limits lowered so that every Winograd layer takes F(2x2) and the deblock the two-step GEMM
    (the >= 2 GiB fallbacks), split included (the F(2x2) filters are packed before either stream runs)."""
    from lidardetection_amd import bev_backbone as bb, wino
    from lidardetection_amd.bev_backbone import FoldedBEVBackbone
    g, h, canvas, pm = _bev_wide_inputs(golden_dir, dev)
    heads = _wide_heads(dev, 256, 31)
    want = g["bev_output"]
    want_head = _heads_fp64(want, heads)
    bev = FoldedBEVBackbone(h.blocks, h.deblocks, heads)
    # the routes: stride-1 3x3 layers on F(4x4), deblock 1 fused, deblock 0 the stride-1 GEMM, first layer from the pillars
    for si in (0, 1):
        convs = bev.stages[si][0]
        assert len(convs) == 2 and convs[0].stride == (2, 2) and convs[0].wino is None
        assert convs[1].wino is not None and convs[1].wino[0] == "f43" and len(convs[1].wino) == 4, si
    (_, up0), (_, up1) = bev.stages
    assert up1.kind == "deconv_mfma" and up1.stride == 2
    assert up0.kind == "gemm" and up0.stride == 1
    assert bev.sparse_first_ok()
    calls = _Calls(monkeypatch, (wino, "conv3x3_f43"), (wino, "conv3x3"), (bb, "deconv_gemm_into_"), (bb, "rows_gemm"),
                   (bb, "gemm_bias_act_into_"))
    monkeypatch.setattr(bb, "_SPLIT", [2])
    for fallback in (False, True):
        if fallback:     # maps "too large" for the F(4x4) kernel and the fused deblock: the >= 2 GiB routes on a small map
            monkeypatch.setattr(wino, "_F43_MAX_BYTES", [1])
            monkeypatch.setattr(bb, "_DECONV_MAX_BYTES", [1])
        for split_min in (8, 1):                                   # B = 2: whole batch, then two part-batches on two streams
            monkeypatch.setattr(bb, "_SPLIT_MIN", [split_min])
            tag = ("fallback" if fallback else "production") + (" split" if split_min == 1 else "")
            _check_folded_entries(bev, canvas, pm, want, want_head, tag, split_min == 1)
            n = calls.take()
            # 4 entries, the split ones run two part-batches: 2 Winograd layers and one fused / two-step deblock per part-batch
            parts = 4 if split_min == 8 else 6
            if fallback:
                assert n["conv3x3_f43"] == 0 and n["conv3x3"] == 2 * parts and n["deconv_gemm_into_"] == 0, (tag, n)
                assert n["rows_gemm"] >= parts, (tag, n)
            else:
                assert n["conv3x3_f43"] == 2 * parts and n["conv3x3"] == 0 and n["deconv_gemm_into_"] == parts, (tag, n)
            assert n["gemm_bias_act_into_"] == parts and bb._LT_GEMM[0], (tag, n)      # the strided-epilogue GEMM ran (and was available)


def _randomize_bn(mods, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in mods.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.empty(mod.num_features).uniform_(-0.3, 0.3, generator=g))
                mod.running_var.copy_(torch.empty(mod.num_features).uniform_(0.6, 1.4, generator=g))
                mod.weight.copy_(torch.empty(mod.num_features).uniform_(0.5, 1.5, generator=g))
                mod.bias.copy_(torch.empty(mod.num_features).uniform_(-0.3, 0.3, generator=g))


@pytest.mark.parametrize("case", ["asymmetric_zero_pad", "dilation", "groups"])
def test_folded_bev_backbone_conv_settings_vs_fp64_stock(dev, golden_dir, case):
    """Conv settings the reference configs do not use but nn.Conv2d / nn.ZeroPad2d allow: the folded backbone computes them (dense
    path: F.pad + conv2d with dilation and groups) and keeps them off the routes that cannot (Winograd, sparse first layer).
    features() from the canvas and merged() from a PillarMap against the fp64 stock modules, 1e-4 of scale."""
    import copy
    import torch.nn as nn
    from lidardetection_amd.bev_backbone import FoldedBEVBackbone
    _, _, canvas, pm = _bev_wide_inputs(golden_dir, dev)
    torch.manual_seed(41)
    zp, pad, dil, groups = {"asymmetric_zero_pad": ((0, 1, 0, 1), 1, 1, 1), "dilation": (1, 2, 2, 1), "groups": (1, 1, 1, 2)}[case]
    blocks = nn.ModuleList([nn.Sequential(
        nn.ZeroPad2d(zp), nn.Conv2d(64, 64, 3, stride=2, padding=0, bias=False), nn.BatchNorm2d(64, eps=1e-3), nn.ReLU(),
        nn.Conv2d(64, 64, 3, padding=pad, dilation=dil, groups=groups, bias=False), nn.BatchNorm2d(64, eps=1e-3), nn.ReLU())])
    deblocks = nn.ModuleList([nn.Sequential(nn.ConvTranspose2d(64, 128, 2, stride=2, bias=False), nn.BatchNorm2d(128, eps=1e-3),
                                            nn.ReLU())])
    _randomize_bn(blocks, 42)
    _randomize_bn(deblocks, 43)
    blocks, deblocks = blocks.eval(), deblocks.eval()
    heads = _wide_heads("cpu", 128, 44)
    with torch.no_grad():                                         # fp64 stock
        xs = canvas.double().cpu()
        for mod in (copy.deepcopy(blocks).double(), copy.deepcopy(deblocks).double()):
            xs = mod[0](xs)
        want = xs.numpy()
        want_head = _heads_fp64(xs, heads)
    blocks, deblocks = blocks.to(dev).to(memory_format=torch.channels_last), deblocks.to(dev).to(memory_format=torch.channels_last)
    heads = [hd.to(dev) for hd in heads]
    bev = FoldedBEVBackbone(blocks, deblocks, heads)
    convs = bev.stages[0][0]
    assert (convs[0].zero_pad, convs[0].pad, convs[1].pad, convs[1].dilation, convs[1].groups) == \
        {"asymmetric_zero_pad": ((0, 1, 0, 1), (0, 0), (1, 1), (1, 1), 1), "dilation": (None, (1, 1), (2, 2), (2, 2), 1),
         "groups": (None, (1, 1), (1, 1), (1, 1), 2)}[case]                  # the settings the stage keeps
    assert convs[1].wino is None or case == "asymmetric_zero_pad"           # no Winograd for dilation / groups
    assert bev.sparse_first_ok() == (case != "asymmetric_zero_pad")          # the neighbour table knows symmetric padding only
    tol, tol_h = 1e-4 * max(1.0, float(np.abs(want).max())), 1e-4 * max(1.0, float(want_head.abs().max()))
    with torch.no_grad():
        got = bev.features(canvas)
        assert tuple(got.shape) == want.shape, (case, tuple(got.shape), want.shape)
        err = float(np.abs(got.cpu().numpy() - want).max())
        got_h = bev.merged(pm)
        err_h = float((got_h.double().cpu() - want_head).abs().max())
    print(f"[conv settings {case}] features {err:.1e} (tol {tol:.1e}) merged(pillars) {err_h:.1e} (tol {tol_h:.1e})")
    assert err <= tol and err_h <= tol_h, (case, err, err_h)


def test_resident_canvas_equals_fresh_scatter_over_successive_frames(dev):
    """ResidentCanvas.update (clear last call's cells, write the new pillars) must leave exactly the canvas a fresh
    PointPillarScatter produces, call after call, including shrinking / growing pillar sets and an invalid row."""
    from lidardetection_amd import pillar_ops
    B, C, ny, nx, cap = 3, 64, 40, 48, 900
    rc = pillar_ops.ResidentCanvas(B, C, ny, nx, cap, dev)
    g = torch.Generator(device="cpu").manual_seed(23)
    for step, n in enumerate((700, 120, 900, 0, 333)):
        cells = torch.randperm(B * ny * nx, generator=g)[:n]
        b, rem = cells // (ny * nx), cells % (ny * nx)
        coords = torch.stack([b, torch.zeros_like(b), rem // nx, rem % nx], 1).int()
        if n > 5:
            coords[3, 0] = B + 2                                         # a row outside the batch: ignored by both paths
        feats = torch.randn(n, C, generator=g)
        pad = cap - n                                                    # device-side count smaller than the buffer
        coords_d = torch.cat([coords, torch.full((pad, 4), 7, dtype=torch.int32)], 0).to(dev)
        feats_d = torch.cat([feats, torch.full((pad, C), 9.0)], 0).to(dev)
        cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        got = rc.update(feats_d, coords_d, num_voxels_dev=cnt)
        want = pillar_ops.pillar_scatter(feats_d, coords_d, B, nx, ny, num_voxels_dev=cnt, channels_last=True)
        assert torch.equal(got, want), step


def test_voxelize_adaptive_fill_over_successive_calls(dev):
    """The LDS-binned path pre-clears only as many rows as the previous call produced (+25 %); rows beyond that are written whole
    by their emit thread.  Alternate sparse and dense batches through ONE voxeliser whose output buffer is poisoned with NaN
    before every call: every row a call reports must be exact (zero padding included)."""
    P, maxv = 32, 16000
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, P, maxv, 4)
    sparse = [synth.cloud_ring(2000 + f) for f in range(3)]
    dense = [synth.cloud_uniform(1000 + f) for f in range(3)]
    tiny = [synth.cloud_uniform(1100 + f)[:500] for f in range(3)]
    for step, frames in enumerate((sparse, dense, sparse, tiny, dense, dense)):
        sizes = [len(f) for f in frames]
        pts = torch.from_numpy(np.concatenate(frames)).to(dev)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        out = vz.alloc_outputs(len(frames), dev)
        out["voxels"].fill_(float("nan"))
        o = vz(pts, offs, 20000, compact=True, out=out)                   # same n_max every call: same workspace
        offsets = o["voxel_offsets"].cpu().numpy()
        for f, pf in enumerate(frames):
            vo, co, nu = c_oracle.voxelize(pf, synth.PP_VOXEL, synth.PP_RANGE, P, maxv)
            a, b = int(offsets[f]), int(offsets[f + 1])
            assert b - a == len(vo), (step, f)
            assert np.array_equal(o["voxels"][a:b].cpu().numpy(), vo), (step, f)
            assert np.array_equal(o["voxel_num_points"][a:b].cpu().numpy(), nu)
            assert np.array_equal(o["voxel_coords"][a:b, 1:].cpu().numpy(), co)
        assert vz.error_flag(len(frames), 20000, dev) == 0


@pytest.mark.parametrize("shape", ["pp", "nus"])
def test_voxelize_resident_output_equals_fresh_output(dev, shape):
    """Resident output buffer (include/lidar_hip.h algo 4, BatchVoxelizer(resident=True)): the zero padding survives from call to
    call and only the previous call's occupied slots are re-zeroed.  Alternating sparse / dense / tiny / empty batches through ONE
    buffer must give, after every call, exactly the sequential oracle's rows on an otherwise ALL-ZERO buffer; a different buffer,
    or a non-resident call in between, must be detected (workspace history) and cleared in full even when it is poisoned."""
    if shape == "pp":
        vs, rng, P, maxv, C = synth.PP_VOXEL, synth.PP_RANGE, 32, 16000, 4
        gen = lambda kind, f: {"sparse": synth.cloud_ring(2000 + f), "dense": synth.cloud_uniform(1000 + f),
                               "tiny": synth.cloud_uniform(1100 + f)[:500], "empty": np.zeros((0, 4), np.float32)}[kind]
        n_max = 20000
    else:
        vs, rng, P, maxv, C = synth.NUS_VOXEL, synth.NUS_RANGE, 10, 60000, 5
        gen = lambda kind, f: {"sparse": synth.cloud_nus(4000 + f)[:9000], "dense": synth.cloud_nus(4100 + f),
                               "tiny": synth.cloud_nus(4200 + f)[:300], "empty": np.zeros((0, 5), np.float32)}[kind]
        n_max = 30000
    B = 3
    vz = BatchVoxelizer(vs, rng, P, maxv, C)
    out = vz.alloc_outputs(B, dev)
    out["voxels"].fill_(float("nan"))                     # the first resident call must clear everything

    def run_and_check(kinds, buf, resident=True, whole_buffer=True):
        frames = [gen(k, f) for f, k in enumerate(kinds)]
        sizes = [len(f) for f in frames]
        pts = torch.from_numpy(np.concatenate(frames) if sum(sizes) else np.zeros((1, C), np.float32)).to(dev)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        o = vz(pts, offs, n_max, compact=True, out=buf, resident=resident)
        offsets = o["voxel_offsets"].cpu().numpy()
        for f, pf in enumerate(frames):
            vo, co, nu = c_oracle.voxelize(pf, vs, rng, P, maxv)
            a, b = int(offsets[f]), int(offsets[f + 1])
            assert b - a == len(vo), (kinds, f)
            assert np.array_equal(o["voxels"][a:b].cpu().numpy().view(np.uint32), vo.view(np.uint32)), (kinds, f)
            assert np.array_equal(o["voxel_num_points"][a:b].cpu().numpy(), nu) and np.array_equal(o["voxel_coords"][a:b, 1:].cpu().numpy(), co)
        if whole_buffer:
            assert not o["voxels"][int(offsets[-1]):].any(), kinds      # everything beyond the produced rows is zero
        return o

    for kinds in (["sparse"] * 3, ["dense"] * 3, ["sparse", "tiny", "dense"], ["tiny"] * 3, ["empty", "dense", "empty"],
                  ["dense"] * 3, ["empty"] * 3, ["sparse"] * 3):
        run_and_check(kinds, out)
    other = vz.alloc_outputs(B, dev)
    other["voxels"].fill_(float("nan"))
    run_and_check(["dense"] * 3, other)                   # another buffer: history does not match -> full clear
    run_and_check(["sparse"] * 3, other)
    out["voxels"].fill_(float("nan"))                     # the old buffer was modified behind the voxeliser's back, but the
    run_and_check(["dense"] * 3, out)                     # history names `other` now: cleared in full again
    # a non-resident call leaves rows beyond its fill extent unspecified: it must invalidate the history
    run_and_check(["tiny"] * 3, out, resident=False, whole_buffer=False)
    out["voxels"][5000:].fill_(float("nan"))              # (those rows are "unspecified" after a non-resident call)
    run_and_check(["dense"] * 3, out)
    assert vz.error_flag(B, n_max, dev) == 0


@pytest.mark.parametrize("limit_offset", [0.0, 0.5])
def test_direction_bin_fixup_known_answers(dev, limit_offset):
    """generate_predicted_boxes' direction fix-up (pcdet/models/dense_heads/anchor_head_template.py:253-266 with
    common_utils.limit_period :52-55): heading = limit_period(rg - DIR_OFFSET, DIR_LIMIT_OFFSET, period) + DIR_OFFSET + period * bin,
    period = 2 pi / NUM_DIR_BINS.  No reference fixture can exist for it (the golden decode has NUM_DIR_BINS = 0), so the expected
    headings are worked out BY HAND in closed form: with DIR_LIMIT_OFFSET = 0 the residue lies in [0, pi) — a heading 0.3 below
    DIR_OFFSET wraps to pi - 0.3 above it; with 0.5 it lies in [-pi/2, pi/2) — the wrap sits at +-pi/2.  Two anchors per location,
    two direction bins (KITTI configs: DIR_OFFSET 0.78539, NUM_DIR_BINS 2), each case with bin 0 and bin 1 winning."""
    from lidardetection_amd import anchor_post
    pi, off = np.pi, 0.78539
    # (rg - DIR_OFFSET, residue for DIR_LIMIT_OFFSET 0, residue for DIR_LIMIT_OFFSET 0.5)
    cases = [(0.3, 0.3, 0.3), (-0.3, pi - 0.3, -0.3), (pi + 0.5, 0.5, 0.5), (-pi - 0.5, pi - 0.5, -0.5), (0.0, 0.0, 0.0),
             (pi / 2 - 1e-3, pi / 2 - 1e-3, pi / 2 - 1e-3), (pi / 2 + 1e-3, pi / 2 + 1e-3, -pi / 2 + 1e-3),
             (-pi / 2 - 1e-3, pi / 2 - 1e-3, pi / 2 - 1e-3), (-pi / 2 + 1e-3, pi / 2 + 1e-3, -pi / 2 + 1e-3),
             (2 * pi + 0.25, 0.25, 0.25), (3.0, 3.0, 3.0 - pi), (-3.0, pi - 3.0, pi - 3.0), (7.5, 7.5 - 2 * pi, 7.5 - 2 * pi)]
    A, nb = 2, 2
    n_loc = len(cases)
    head = np.zeros((1, n_loc, A * 7 + A * nb), np.float32)
    anchors = np.zeros((n_loc * A, 7), np.float32)
    anchors[:, 3:6] = [3.9, 1.6, 1.56]
    want = np.zeros((n_loc * A,), np.float64)
    for i, (val, r0, r5) in enumerate(cases):
        for a in range(A):
            ra = np.float32(0.0 if a == 0 else 1.57)                     # the two anchor rotations of the KITTI configs
            anchors[i * A + a, 6] = ra
            head[0, i, a * 7 + 6] = np.float32(np.float32(off) + np.float32(val)) - ra     # encoded angle: rg = t + ra = off + val
            lab = (i + a) % 2
            head[0, i, A * 7 + a * nb + lab] = 1.0                       # that bin's logit wins
            want[i * A + a] = (r0 if limit_offset == 0.0 else r5) + off + pi * lab
    idx = torch.arange(n_loc * A, device=dev).view(1, -1)
    boxes = anchor_post.decode_topk(torch.from_numpy(head).to(dev), idx, torch.from_numpy(anchors).to(dev), A, box_off=0, dir_off=A * 7,
                                    num_dir_bins=nb, dir_offset=off, dir_limit_offset=limit_offset)
    got = boxes[0, :, 6].cpu().numpy().astype(np.float64)
    # fp32 evaluation of a closed form: a few ulp of values up to ~10 (the exact-zero case (0.0, ...) sits on a floor() boundary
    # and is placed so that fp32 rounding cannot cross it: rg - DIR_OFFSET == 0 exactly)
    np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)
    assert np.array_equal(boxes[0, :, 3:6].cpu().numpy(), anchors[:, 3:6])      # exp(0) * size: untouched by the fix-up
