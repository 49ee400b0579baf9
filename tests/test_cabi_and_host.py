"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol declared in
include/lidar_hip.h, the ctypes table matches the header, pure-host queries work, and the product has no
CPU fallback (ops raise on CPU tensors).  No compute kernels are launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lidardetection_amd import _lib, synth
from lidardetection_amd.voxelizer import BatchVoxelizer, grid_size_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lidar_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lidar_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported_and_bound():
    names = _declared()
    assert len(names) >= 10
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/lidar_hip.h but not exported by liblidar_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in lidardetection_amd/_lib.py"
    for n in _lib.SIGNATURES:
        assert n in names, f"{n} bound in _lib.py but not declared in the header"
    _lib.lib()  # resolves + types every symbol


def test_bound_types_are_the_parsed_header():
    """every function of the loaded library carries exactly the types parse_header reads from the header, and LIMITS its constants"""
    sigs, limits = _lib.parse_header(open(os.path.join(ROOT, "include", "lidar_hip.h")).read())
    assert sorted(sigs) == _declared() and sigs == _lib.SIGNATURES and limits == _lib.LIMITS
    L = _lib.lib()
    for n, (res, args) in sigs.items():
        fn = getattr(L, n)
        assert fn.restype is res and list(fn.argtypes) == args, n


vp, i32, i64, f32, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
# typed by hand from the header's text, one for each kind of type the parser maps: the parser cannot be wrong and these still hold
PINNED = {
    "lidar_voxelize_workspace_bytes": (sz, [i32, i32, i32]),                                  # size_t return
    "lidar_timer_destroy": (None, [vp]),                                                      # void return
    "lidar_timer_create": (vp, []),                                                           # pointer return, (void) list
    "lidar_nms_mask_ptr": (vp, [vp, i32, i32]),                                               # const pointer return
    "lidar_timer_elapsed_ms": (f32, [vp]),                                                    # float return
    "lidar_optim_plan": (i64, [vp, i32, vp, vp, i64]),                                        # long long return
    "lidar_optim_adam_step": (i32, [vp, i32, vp, vp, i64, vp, f64, f64, f64, f64, f64, i64, i32, vp]),      # double parameters
    "lidar_ball_query_stack2": (i32, [i32, i32, f32, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp]),           # float parameters
    "lidar_head_rows": (i32, [vp, vp, i32, i32, i64, i32, vp, i32, vp, i32, i32, i32, i32, vp, i32, i64, vp, vp]),
    "lidar_bn_relu_train_workspace_bytes": (sz, [i64, i32]),
    "lidar_bn_relu_train_forward": (i32, [i32, vp, vp, vp, vp, i64, vp, vp, f32, vp, i32, i32, vp, vp, vp, vp, sz, vp]),   # void *const *x
    "lidar_voxelize_cpu": (i32, [vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz]),    # size_t last, no stream
}
# the two longest lists: length, and where their arguments are not pointers
PINNED_LONG = {
    "lidar_augment": (39, {2: i32, 3: i32, 6: i32, 7: i32, 12: i32, 13: i32, 15: i32, 16: i32, 27: i32, 28: i32, 29: i64, 30: i32, 37: sz}),
    "lidar_kitti_eval_class": (32, {0: i32, 10: i32, 11: i64, 12: i64, 13: i64, 14: i32, 15: i32, 17: i32, 19: i32, 21: i32, 22: i32,
                                    30: sz}),
}


def test_signatures_pinned_by_hand():
    for n, sig in PINNED.items():
        assert _lib.SIGNATURES[n] == sig, n
    for n, (count, scalars) in PINNED_LONG.items():
        res, args = _lib.SIGNATURES[n]
        assert res is i32 and len(args) == count, n
        assert {i: a for i, a in enumerate(args) if a is not vp} == scalars, n
    assert {k: _lib.LIMITS[k] for k in ("LIDAR_OK", "LIDAR_ERR_ARG", "LIDAR_ERR_LAUNCH", "LIDAR_ERR_WORKSPACE", "LIDAR_ERR_UNSUPPORTED")} == {
        "LIDAR_OK": 0, "LIDAR_ERR_ARG": -1, "LIDAR_ERR_LAUNCH": -2, "LIDAR_ERR_WORKSPACE": -3, "LIDAR_ERR_UNSUPPORTED": -4}
    assert _lib.LIMITS["LIDAR_POINT_HEAD_MAX_POINTS"] == 1 << 20 and _lib.LIMITS["LIDAR_KITTI_EVAL_MAX_TOTAL_DT"] == 1 << 22
    assert _lib.LIMITS["LIDAR_PFN_TRAIN_STATS_DOUBLES"] == 272 and "LIDAR_HIP_H" not in _lib.LIMITS


def test_workspace_queries_are_pure_host():
    L = _lib.lib()
    assert L.lidar_voxelize_workspace_bytes(16, 20000, 16000) > 16 * 20000 * 4
    assert L.lidar_voxelize_workspace_bytes(0, 10, 10) == 0
    assert L.lidar_nms_workspace_bytes(1, 4096) >= 4096 * 64 * 8
    assert L.lidar_pillar_scatter_workspace_bytes(2, 432, 496) >= 2 * 432 * 496 * 4
    assert L.lidar_iou_workspace_bytes(10, 20) > 0


def test_argument_errors_return_status_not_exit():
    L = _lib.lib()
    # null pointers / bad sizes are rejected before any launch (reference: fprintf + exit(-1))
    assert L.lidar_boxes_pairwise_bev(None, 3, None, 3, 1, None, None, 0, None) == -1
    assert L.lidar_nms_batch(None, None, 0, 10, 0.1, 0, None, None, None, 0, None) == -1
    assert L.lidar_mean_vfe(None, None, 5, 5, 4, 0, None, None) == -1


def test_grid_size_matches_reference_configs():
    assert grid_size_of(synth.PP_VOXEL, synth.PP_RANGE).tolist() == [432, 496, 1]      # pointpillar.yaml
    assert grid_size_of(synth.SEC_VOXEL, synth.SEC_RANGE).tolist() == [1408, 1600, 40]  # kitti_dataset.yaml
    assert grid_size_of(synth.NUS_VOXEL, synth.NUS_RANGE).tolist() == [1024, 1024, 40]  # nuscenes_dataset.yaml


def test_no_cpu_fallback():
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 100)
    with pytest.raises(_lib.LidarHipError):
        vz(torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32), 10)
    from lidardetection_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
    with pytest.raises(_lib.LidarHipError):
        iou3d_nms_utils.nms_gpu(torch.zeros(4, 7), torch.zeros(4), 0.1)


def test_synthetic_generators_are_seeded():
    a, b = synth.cloud_uniform(1000), synth.cloud_uniform(1000)
    assert a.shape == (20000, 4) and np.array_equal(a, b)
    r = synth.cloud_ring(2000)
    assert r.shape == (64 * 312, 4)
    bx, sc = synth.boxes_nms(3000)
    assert bx.shape == (4096, 7) and len(np.unique(sc)) == 4096


def test_cpu_entry_points_bit_exact_vs_reference_golden(golden_dir):
    """boxes_iou_bev_cpu / points_in_boxes_cpu (host code in the product library) vs the reference's own compiled CPU
    functions (tests/golden/iou3d_ref.npz) — these run without a GPU, as they do in the reference's DataLoader workers."""
    from lidardetection_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
    from lidardetection_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    g = np.load(os.path.join(golden_dir, "iou3d_ref.npz"))
    iou = iou3d_nms_utils.boxes_bev_iou_cpu(g["boxes_a"], g["boxes_b"])            # numpy in -> numpy out
    assert isinstance(iou, np.ndarray) and np.array_equal(iou.view(np.uint32), g["iou_bev_cpu"].view(np.uint32))
    iou_t = iou3d_nms_utils.boxes_bev_iou_cpu(torch.from_numpy(g["nms_boxes_sorted"]), torch.from_numpy(g["nms_boxes_sorted"]))
    assert np.array_equal(iou_t.numpy().view(np.uint32), g["nms_iou_bev_cpu"].view(np.uint32))
    pib = roiaware_pool3d_utils.points_in_boxes_cpu(g["pib_points"], g["boxes_a"])
    ref = np.unpackbits(g["pib_cpu"], axis=1)[:, :g["pib_shape"][1]].astype(np.int32)
    assert np.array_equal(pib, ref)


def _ref_checks():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ref_checks.json")) as fh:
        return json.load(fh)


def test_reference_backbone_source_runs_on_this_spconv():
    """Drop-in check of the spconv mirror: the REFERENCE's own pcdet/models/backbones_3d/spconv_backbone.py, loaded from its
    file with `spconv` aliased to lidardetection_amd.spconv, builds both backbones
    (tests/golden/make_golden.py ref_checks), and their state_dicts (names + shapes = checkpoint layout), num_point_features
    and sparse_shape, stored in tests/golden/ref_checks.json, equal this repo's mirror."""
    from lidardetection_amd.pcdet.models.backbones_3d import spconv_backbone as mine
    from lidardetection_amd.pcdet.utils.cfg import AttrDict
    ref = _ref_checks()["spconv_backbones"]
    assert sorted(ref) == ["VoxelBackBone8x", "VoxelResBackBone8x"]
    for name, a in ref.items():
        b = getattr(mine, name)(AttrDict(), 4, np.array([1408, 1600, 40]))     # the reference passes a numpy grid size
        sb = b.state_dict()
        assert [k for k, _ in a["state_dict"]] == list(sb.keys()), name
        assert all(list(sb[k].shape) == shape for k, shape in a["state_dict"]), name
        assert a["num_point_features"] == b.num_point_features
        assert a["sparse_shape"] == [int(v) for v in b.sparse_shape]


def test_every_native_symbol_the_reference_wrappers_call_is_exported():
    """Static drop-in check: the `<native module>.<function>(` calls in the reference's operator wrappers (scanned from their
    source by tests/golden/make_golden.py ref_checks into tests/golden/ref_checks.json) must each be a function on this
    repo's same-named ext module.  (The wrappers themselves cannot be imported: pcdet.utils.common_utils needs the absent
    `quaternion` package.)"""
    from lidardetection_amd.ext import (iou3d_nms_cuda, pointnet2_batch_cuda, pointnet2_stack_cuda, roiaware_pool3d_cuda,
                                        roipoint_pool3d_cuda)
    mods = {"pcdet/ops/iou3d_nms/iou3d_nms_utils.py": iou3d_nms_cuda,
            "pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py": roiaware_pool3d_cuda,
            "pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py": roipoint_pool3d_cuda,
            "pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py": pointnet2_stack_cuda,
            "pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py": pointnet2_batch_cuda}
    calls = _ref_checks()["native_calls"]
    assert sorted(c["wrapper"] for c in calls) == sorted(mods)
    total = 0
    for c in calls:
        names = c["functions"]
        assert names, c["wrapper"]
        missing = sorted(n for n in names if not callable(getattr(mods[c["wrapper"]], n, None)))
        assert not missing, (c["wrapper"], missing)
        total += len(names)
    assert total >= 20


def _cases_for_host_voxel_generator():
    r = np.random.default_rng(21)
    dense = synth.cloud_uniform(1002, n=5000)
    dense[:, :2] = dense[:, :2] * 0.02 + np.array([10.0, 0.0], np.float32)           # ~100 points per pillar: the P cap
    lo, hi = np.array(synth.PP_RANGE[:3], np.float32), np.array(synth.PP_RANGE[3:], np.float32)
    edges = np.array([[lo[0], lo[1], lo[2], 0.1], [hi[0], 0, 0, 0.2], [np.nextafter(hi[0], -np.inf, dtype=np.float32), 0, 0, 0.3],
                      [-0.001, 0, 0, 0.4], [5, 5, 1.0, 0.5], [5, 5, 0.999, 0.6], [0.16, 0.16, 0, 0.8], [0.15999, 0.16, 0, 0.9],
                      [np.nan, 0, 0, 1.0], [1e9, 0, 0, 1.0]], np.float32)
    ring = synth.cloud_ring(2002)
    return [
        ("pp ring shuffled", ring[r.permutation(len(ring))], synth.PP_VOXEL, synth.PP_RANGE, 32, 16000),
        ("pp uniform, voxel cap", synth.cloud_uniform(1000), synth.PP_VOXEL, synth.PP_RANGE, 32, 16000),
        ("pp dense pillars, P cap", dense, synth.PP_VOXEL, synth.PP_RANGE, 32, 16000),
        ("P = 1, tiny cap", dense, synth.PP_VOXEL, synth.PP_RANGE, 1, 50),
        ("second", synth.cloud_ring(2000), synth.SEC_VOXEL, synth.SEC_RANGE, 5, 16000),
        ("nuscenes, 5 features", synth.cloud_nus(4000), synth.NUS_VOXEL, synth.NUS_RANGE, 10, 60000),
        ("edges / NaN / far", edges, synth.PP_VOXEL, synth.PP_RANGE, 32, 16000),
        ("empty", np.zeros((0, 4), np.float32), synth.PP_VOXEL, synth.PP_RANGE, 32, 16000),
    ]


def test_host_voxel_generator_bit_exact_vs_oracle_and_reference_call_pattern():
    """spconv.utils.VoxelGeneratorV2 / VoxelGenerator .generate(numpy) — the reference's DataLoader-worker call
    (pcdet/datasets/processor/data_processor.py:48-80) — runs lidar_voxelize_cpu (csrc/cpu_ops.hip: own hash-map scan, no GPU,
    no oracle): dict / tuple outputs bit-exact vs the sequential oracle on PointPillar / SECOND / NuScenes shapes, caps, edge
    points and an empty frame."""
    from lidardetection_amd.spconv.utils import VoxelGenerator, VoxelGeneratorV2
    from oracle import c_oracle
    for name, pts, vs, rng, P, mv in _cases_for_host_voxel_generator():
        ev, ec, en = c_oracle.voxelize(pts, vs, rng, P, mv)
        g2 = VoxelGeneratorV2(voxel_size=vs, point_cloud_range=rng, max_num_points=P, max_voxels=mv)
        out = g2.generate(pts)
        assert isinstance(out, dict) and out["voxel_num"] == len(ev), name
        assert out["voxels"].dtype == np.float32 and out["coordinates"].dtype == np.int32
        assert np.array_equal(out["voxels"].view(np.uint32), ev.view(np.uint32)), name
        assert np.array_equal(out["coordinates"], ec) and np.array_equal(out["num_points_per_voxel"], en), name
        assert np.array_equal(out["voxel_point_mask"][:, :, 0] > 0, np.arange(P)[None, :] < en[:, None]), name
        v, c, n = VoxelGenerator(voxel_size=vs, point_cloud_range=rng, max_num_points=P, max_voxels=mv).generate(pts)
        assert np.array_equal(v, ev) and np.array_equal(c, ec) and np.array_equal(n, en), name
        assert g2.grid_size.tolist() == np.round((np.array(rng[3:]) - np.array(rng[:3])) / np.array(vs)).astype(np.int64).tolist()


def _generate_in_child(q, pts):
    from lidardetection_amd.spconv.utils import VoxelGeneratorV2
    out = VoxelGeneratorV2(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000).generate(pts)
    q.put((out["voxels"], out["coordinates"], out["num_points_per_voxel"]))


def test_host_voxel_generator_runs_in_a_forked_worker():
    """the reference's DataLoader workers are forked children: generate() must work there (it touches no GPU state)"""
    import multiprocessing as mp
    from oracle import c_oracle
    from lidardetection_amd import _lib
    _lib.lib()                                             # parent has the library loaded, like a training process
    pts = synth.cloud_ring(2004)
    ctx = mp.get_context("fork")
    q = ctx.Queue()
    p = ctx.Process(target=_generate_in_child, args=(q, pts))
    p.start()
    v, c, n = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    ev, ec, en = c_oracle.voxelize(pts, synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)
    assert np.array_equal(v, ev) and np.array_equal(c, ec) and np.array_equal(n, en)


def test_trim_padding_cuts_capacity_sized_tensors_to_their_true_rows():
    """host logic of the read-back-free sparse forward (spconv/modules.py:_trim_padding): capacity-sized outputs and rulebook
    tables become prefix views of their true row counts, SubM tables keep nbr_t aliased to nbr, cached row orders (which cover
    the padding rows) are dropped, exact-sized tensors are left alone."""
    import torch
    from lidardetection_amd.spconv import modules
    from lidardetection_amd.spconv.tensor import SparseConvTensor
    c1 = torch.arange(40, dtype=torch.int32).view(10, 4)            # level 1: exact (10 rows)
    c2 = torch.arange(64, dtype=torch.int32).view(16, 4)            # level 2: capacity 16, true 11
    f2 = torch.randn(16, 8)
    nbr_conv, nbr_sub2 = torch.zeros(16, 27, dtype=torch.int32), torch.ones(16, 27, dtype=torch.int32)
    idict = {"__grid_token__": {"token": 1},
             "spconv2": {"subm": False, "nbr": nbr_conv, "nbr_t": None, "in_indices": c1, "out_indices": c2, "order": [1, 2, None]},
             "subm2": {"subm": True, "nbr": nbr_sub2, "nbr_t": nbr_sub2, "in_indices": c2, "out_indices": c2, "order": [1, 2, None]},
             "subm1": {"subm": True, "nbr": torch.zeros(10, 27, dtype=torch.int32), "nbr_t": None, "in_indices": c1, "out_indices": c1,
                       "order": "kept"}}
    idict["subm1"]["nbr_t"] = idict["subm1"]["nbr"]
    x1, x2 = SparseConvTensor(torch.randn(10, 4), c1, [4, 4, 4], 1), SparseConvTensor(f2, c2, [2, 2, 2], 1)
    modules._trim_padding([x1, x2], idict, {c2.data_ptr(): 11})
    assert x1.features.shape[0] == 10 and x2.features.shape[0] == 11 and x2.indices.shape[0] == 11
    assert x2.features.data_ptr() == f2.data_ptr() and torch.equal(x2.indices, c2[:11])
    assert idict["spconv2"]["nbr"].shape == (11, 27) and idict["spconv2"]["out_indices"].shape[0] == 11
    assert idict["spconv2"]["in_indices"].shape[0] == 10 and "order" not in idict["spconv2"]
    assert idict["subm2"]["nbr"].shape == (11, 27) and idict["subm2"]["nbr_t"] is idict["subm2"]["nbr"] and "order" not in idict["subm2"]
    assert idict["subm1"]["nbr"].shape == (10, 27) and idict["subm1"]["order"] == "kept"


def test_winograd_and_deblock_size_predicates(monkeypatch):
    """wino.f43_fits / bev_backbone.deconv_fits decide, on the host alone, when a map is too large for the 32-bit byte offsets of
    the F(4x4, 3x3) kernel and of the fused deblock (lidar_wino43_conv3x3_nhwc / lidar_deconv_gemm_nhwc refuse >= 2^31 - 1 bytes).
    The output counts whether or not the caller passes it: SECOND-MultiHead's merged first branch layer (64 -> 2304 channels on
    128 x 128) at bs 16 has a small input and a 2.4 GB output, allocated by conv3x3_auto itself."""
    import torch
    from lidardetection_amd import bev_backbone, wino

    def no_library():
        raise AssertionError("the size predicates must not load the HIP library")
    monkeypatch.setattr(_lib, "lib", no_library)
    assert not wino.f43_fits((16, 64, 128, 128), 2304)                     # SECOND-MultiHead bs 16, out=None
    assert wino.f43_fits((14, 64, 128, 128), 2304)                         # 2.11e9 bytes: still under 2^31 - 1
    assert not wino.f43_fits((15, 64, 128, 128), 2304)
    # PointPillar-KITTI bs 16: the stride-1 layers of the three blocks (248 x 216, 124 x 108, 62 x 54) and SECOND's 200 x 176 ones
    for shape, cout in (((16, 64, 248, 216), 64), ((16, 128, 124, 108), 128), ((16, 256, 62, 54), 256),
                        ((16, 128, 200, 176), 128), ((16, 256, 100, 88), 256)):
        assert wino.f43_fits(shape, cout), shape
    big_out = torch.empty((16, 2304, 128, 128), device="meta")              # shape only, nothing allocated
    small_out = torch.empty((16, 64, 128, 128), device="meta")
    assert not wino.f43_fits((16, 64, 128, 128), 64, out=big_out)           # a caller-supplied output that is too large
    assert wino.f43_fits((16, 64, 128, 128), 64, out=small_out)
    assert not wino.f43_fits((16, 2304, 128, 128), 64)                      # ... or an input that is
    # the limit is the module-level one (tests lower it to reach the fallback on small maps)
    monkeypatch.setattr(wino, "_F43_MAX_BYTES", [2 * 64 * 8 * 8 * 4 + 1])
    assert wino.f43_fits((2, 64, 8, 8), 64) and not wino.f43_fits((2, 64, 8, 8), 128)
    # fused deblock: PointPillar bs 16 (128 x 124 x 108 -> 384 x 248 x 216 concat map) fits, 2.4 GB of concat map does not
    assert bev_backbone.deconv_fits(16, 128, 124, 108, 2, 384)
    assert not bev_backbone.deconv_fits(16, 256, 100, 88, 2, 1024)
    monkeypatch.setattr(bev_backbone, "_DECONV_MAX_BYTES", [2 * 64 * 6 * 5 * 4 * 4])
    assert not bev_backbone.deconv_fits(2, 64, 6, 5, 2, 64) and bev_backbone.deconv_fits(2, 64, 6, 5, 2, 63)
