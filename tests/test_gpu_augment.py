"""GPU checks of the train-time augmentation (csrc/augment.hip through lidardetection_amd/augment.py and the raw C ABI): every case
of tests/golden/augment_ref.npz (written by the reference itself), edge shapes against the numpy restatement (tests/_augment_np.py)
with inputs drawn under the golden file's borderline condition, bitwise reproducibility, graph capture, shuffle_points, and the path
into the voxeliser and PointPillarKITTI.train_loss.  Counts, offsets, sample_valid and row orders compare exactly; coordinates and
boxes to the project's stated 1e-4, |a - b| <= 1e-4 * max(1, |b|)."""
import numpy as np
import pytest
import torch

import _augment_np as anp
from lidardetection_amd import _lib, augment, synth
from lidardetection_amd.voxelizer import BatchVoxelizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _device_inputs(inp):
    return _up(inp["points"], np.float32), _up(inp["point_offsets"], np.int32), _up(inp["gt_boxes"], np.float32), _up(inp["gt_counts"], np.int32)


def _augmentor(inp, cfg):
    db = augment.GtDatabase(inp["db_points"], inp["db_offsets"], inp["db_boxes"], inp["db_cls"], device=DEV)
    aug = augment.TrainAugmentor(db, inp["cand"].shape[1], cfg["pc_range"], remove_extra_width=cfg["remove_extra_width"],
                                 collide_extra_width=cfg.get("collide_extra_width"), remove_outside_boxes=cfg["remove_outside_boxes"],
                                 min_num_corners=cfg["min_num_corners"], sample_rot_range=(0, 0) if "sample_rot" in inp else None)
    return aug


def _run(inp, cfg, aug=None, **kw):
    aug = aug or _augmentor(inp, cfg)
    return aug(*_device_inputs(inp), inp["cand"], planes=inp.get("plane"), flip_x=inp["flip_x"], flip_y=inp["flip_y"], rot=inp["rot"],
               scale=inp["scale"], sample_rot=inp.get("sample_rot"), **kw)


def _host(out):
    offs = out["point_offsets"].cpu().numpy()
    return dict(points=out["points"][:int(offs[-1])].cpu().numpy(), point_offsets=offs, gt_boxes=out["gt_boxes"].cpu().numpy(),
                gt_counts=out["gt_counts"].cpu().numpy(), sample_valid=out["sample_valid"].cpu().numpy())


def _compare(got, exp):
    for k in ("point_offsets", "gt_counts", "sample_valid"):
        print(k, got[k].reshape(-1)[:24], exp[k].reshape(-1)[:24])
        assert np.array_equal(got[k], exp[k]), k
    print("max |d points|", np.abs(got["points"] - exp["points"]).max(initial=0), "max |d boxes|", np.abs(got["gt_boxes"] - exp["gt_boxes"]).max(initial=0))
    assert anp.close(got["points"], exp["points"]) and anp.close(got["gt_boxes"], exp["gt_boxes"])
    assert np.array_equal(got["points"][:, 3:], exp["points"][:, 3:])                # kept-row order: the features are copied bits
    assert np.array_equal(got["gt_boxes"][..., 7], exp["gt_boxes"][..., 7])          # box row order and the zero padding


@pytest.mark.parametrize("name", anp.CASES)
def test_golden_through_train_augmentor(name):
    cfg, inp, exp, _ = anp.load_contract(name)
    out = _run(inp, cfg, host_offsets=inp["point_offsets"])
    _compare(_host(out), exp)
    assert out["n_max"] >= int(np.diff(exp["point_offsets"]).max())


@pytest.mark.parametrize("name", anp.CASES)
def test_golden_through_the_c_abi(name):
    cfg, inp, exp, _ = anp.load_contract(name)
    L = _lib.lib()
    B, G, S = inp["cand"].shape
    M, C, n = inp["gt_boxes"].shape[1], inp["points"].shape[1], inp["points"].shape[0]
    sizes = np.diff(inp["db_offsets"])
    bound = int(np.where(inp["cand"] >= 0, sizes[np.maximum(inp["cand"], 0)], 0).sum())
    cap = n + bound + 7
    pts, offs, gt, cnt = _device_inputs(inp)
    dbp, dbo, dbb, dbc = _up(inp["db_points"], np.float32), _up(inp["db_offsets"], np.int32), _up(inp["db_boxes"], np.float32), _up(inp["db_cls"], np.int32)
    rot64 = inp["rot"].astype(np.float64)
    t = dict(cand=_up(inp["cand"], np.int32), fx=_up(inp["flip_x"], np.int32), fy=_up(inp["flip_y"], np.int32), rot=_up(inp["rot"], np.float32),
             cs=_up(np.stack([np.cos(rot64), np.sin(rot64)], 1), np.float32), sc=_up(inp["scale"], np.float32),
             sr=_up(inp.get("sample_rot"), np.float32), pl=_up(inp.get("plane"), np.float32))
    o = dict(points=torch.full((cap, C), -7.0, device=DEV), point_offsets=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
             gt_boxes=torch.full((B, M + G * S, 8), -7.0, device=DEV), gt_counts=torch.zeros(B, dtype=torch.int32, device=DEV),
             sample_valid=torch.full((B, G, S), -7, dtype=torch.int32, device=DEV))
    nbytes = int(L.lidar_augment_workspace_bytes(B, G, S, cap))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cw = cfg.get("collide_extra_width")

    def call(ws_bytes, cap_arg):
        return L.lidar_augment(_lib.ptr(pts), _lib.ptr(offs), n, C, _lib.ptr(gt), _lib.ptr(cnt), B, M, _lib.ptr(dbp), _lib.ptr(dbo),
                               _lib.ptr(dbb), _lib.ptr(dbc), len(sizes), int(inp["db_points"].shape[0]), _lib.ptr(t["cand"]), G, S,
                               _lib.ptr(t["fx"]), _lib.ptr(t["fy"]), _lib.ptr(t["rot"]), _lib.ptr(t["cs"]), _lib.ptr(t["sc"]), _lib.ptr(t["sr"]),
                               _lib.ptr(t["pl"]), _lib.host_f32(cfg["remove_extra_width"]), None if cw is None else _lib.host_f32(cw),
                               _lib.host_f32(cfg["pc_range"]), 1, cfg["min_num_corners"], bound, cap_arg, _lib.ptr(o["points"]),
                               _lib.ptr(o["point_offsets"]), _lib.ptr(o["gt_boxes"]), _lib.ptr(o["gt_counts"]), _lib.ptr(o["sample_valid"]),
                               _lib.ptr(ws), ws_bytes, _lib.stream())

    assert call(nbytes - 1, cap) == -3 and call(nbytes, n + bound - 1) == -1          # refused before any launch
    assert float(o["gt_boxes"].max()) == -7.0
    assert call(nbytes, cap) == 0
    got = _host(o)
    _compare(got, exp)
    assert float(o["points"][int(got["point_offsets"][-1]):].max()) == -7.0           # nothing is written past the last row


EDGE = {
    "frame_sizes": dict(frame_points=[1, 0, 255, 256, 257]),
    "past_scan_tile": dict(frame_points=[256 * 256 + 1, 300], n_db=40, S=10, still=True),
    "no_candidates": dict(frame_points=[300, 200], all_minus_one=True),
    "s0": dict(frame_points=[300, 200], S=0),
    "boxes_512": dict(frame_points=[200, 100], M=8, G=8, S=63, n_db=144, n_gt=8),
    "c3": dict(frame_points=[300, 257], C=3),
    "c8": dict(frame_points=[300, 257], C=8),
    "plain": dict(frame_points=[400, 300, 200], plane=False, sample_rot=False, collide=False, scale=False),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes_against_the_restatement(name):
    spec = dict(EDGE[name])
    all_minus_one = spec.pop("all_minus_one", False)
    inp, cfg = anp.synth_inputs(sum(map(ord, name)), **spec)
    if all_minus_one:
        inp["cand"][:] = -1
    assert (np.diff(inp["db_offsets"]) == 0).any() or inp["cand"].shape[2] == 0        # an object of 0 points
    exp = anp.augment(inp, cfg)
    aug = _augmentor(inp, cfg)
    aug.apply_scale = cfg["apply_scale"]
    got = _host(_run(inp, cfg, aug))
    _compare(got, exp)
    if name == "boxes_512":
        assert inp["gt_boxes"].shape[1] + inp["cand"].shape[1] * inp["cand"].shape[2] == 512 and exp["sample_valid"].sum() > 100


def test_batch_of_zero_frames():
    inp, cfg = anp.synth_inputs(5, [10])
    aug = _augmentor(inp, cfg)
    out = aug(torch.zeros((0, 4), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros((0, 8, 8), device=DEV),
              torch.zeros(0, dtype=torch.int32, device=DEV), np.zeros((0, 3, 15), np.int32), flip_x=np.zeros(0), flip_y=np.zeros(0),
              rot=np.zeros(0), scale=np.zeros(0), sample_rot=np.zeros((0, 3, 15)))
    assert out["points"].shape == (0, 4) and out["point_offsets"].tolist() == [0] and out["gt_boxes"].shape == (0, 8 + 45, 8)
    assert out["n_max"] == 0


def test_two_calls_are_bitwise_identical_and_a_graph_replays_them():
    cfg, inp, exp, _ = anp.load_contract("wide")
    aug = _augmentor(inp, cfg)
    a, b = _host(_run(inp, cfg, aug)), _host(_run(inp, cfg, aug))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # capture the raw call (the wrapper's uploads are not part of it), replay once
    args = _device_inputs(inp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = _run(inp, cfg, aug)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    up = {k: _up(inp[k], d) for k, d in (("cand", np.int32), ("flip_x", np.int32), ("flip_y", np.int32), ("rot", np.float32),
                                         ("scale", np.float32), ("sample_rot", np.float32))}
    rot64 = inp["rot"].astype(np.float64)
    cs = _up(np.stack([np.cos(rot64), np.sin(rot64)], 1), np.float32)
    L, db = _lib.lib(), aug.db
    B, G, S = inp["cand"].shape
    M, n = inp["gt_boxes"].shape[1], inp["points"].shape[0]
    cap = int(warm["points"].shape[0])
    o = {k: torch.zeros_like(v) for k, v in warm.items() if torch.is_tensor(v)}
    ws = torch.empty(int(L.lidar_augment_workspace_bytes(B, G, S, cap)), dtype=torch.uint8, device=DEV)
    with torch.cuda.graph(graph):
        status = L.lidar_augment(_lib.ptr(args[0]), _lib.ptr(args[1]), n, 4, _lib.ptr(args[2]), _lib.ptr(args[3]), B, M, _lib.ptr(db.points),
                                 _lib.ptr(db.offsets), _lib.ptr(db.boxes), _lib.ptr(db.cls), db.n_obj, int(db.points.shape[0]),
                                 _lib.ptr(up["cand"]), G, S, _lib.ptr(up["flip_x"]), _lib.ptr(up["flip_y"]), _lib.ptr(up["rot"]), _lib.ptr(cs),
                                 _lib.ptr(up["scale"]), _lib.ptr(up["sample_rot"]), None, _lib.host_f32(cfg["remove_extra_width"]),
                                 _lib.host_f32(cfg["collide_extra_width"]), _lib.host_f32(cfg["pc_range"]), 1, cfg["min_num_corners"],
                                 cap - n, cap, _lib.ptr(o["points"]), _lib.ptr(o["point_offsets"]), _lib.ptr(o["gt_boxes"]),
                                 _lib.ptr(o["gt_counts"]), _lib.ptr(o["sample_valid"]), _lib.ptr(ws), ws.numel(), _lib.stream())
    assert status == 0
    graph.replay()
    torch.cuda.synchronize()
    c = _host(o)
    for k in a:
        assert np.array_equal(a[k], c[k]), k


def test_shuffle_points():
    cfg, inp, exp, _ = anp.load_contract("kitti")
    aug = _augmentor(inp, cfg)
    plain = _host(_run(inp, cfg, aug))
    cap = inp["points"].shape[0] + int(np.where(inp["cand"] >= 0, np.diff(inp["db_offsets"])[np.maximum(inp["cand"], 0)], 0).sum())
    keys = np.random.default_rng(3).random(cap).astype(np.float32)
    one, two = _host(_run(inp, cfg, aug, shuffle=True, shuffle_keys=keys)), _host(_run(inp, cfg, aug, shuffle=True, shuffle_keys=keys))
    assert np.array_equal(one["point_offsets"], plain["point_offsets"]) and np.array_equal(one["points"], two["points"])
    offs = plain["point_offsets"]
    for b in range(len(offs) - 1):
        p, q = plain["points"][offs[b]:offs[b + 1]], one["points"][offs[b]:offs[b + 1]]
        order = np.lexsort((np.arange(len(p)), keys[offs[b]:offs[b + 1]]))
        assert np.array_equal(q, p[order])                                           # ascending (key, row) within the frame
        assert len(p) < 2 or not np.array_equal(p, q)
    drawn = _host(_run(inp, cfg, aug, shuffle=True, rng=np.random.default_rng(1)))
    assert np.array_equal(drawn["point_offsets"], offs)
    for b in range(len(offs) - 1):
        assert np.array_equal(np.sort(drawn["points"][offs[b]:offs[b + 1]].view("V16"), axis=0),
                              np.sort(plain["points"][offs[b]:offs[b + 1]].view("V16"), axis=0))


def test_into_the_voxeliser_and_train_loss():
    cfg, inp, exp, _ = anp.load_contract("kitti")
    two = dict(inp)                          # the first two frames of the case: frames are independent
    n2 = int(inp["point_offsets"][2])
    two.update(points=inp["points"][:n2], point_offsets=inp["point_offsets"][:3])
    for k in ("gt_boxes", "gt_counts", "cand", "flip_x", "flip_y", "rot", "scale", "plane"):
        two[k] = inp[k][:2]
    out = _run(two, cfg)
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)
    mine = vz(out["points"], out["point_offsets"], out["n_max"])
    e2 = int(exp["point_offsets"][2])
    ref_pts, ref_offs = _up(exp["points"][:e2], np.float32), _up(exp["point_offsets"][:3], np.int32)
    theirs = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)(ref_pts, ref_offs, int(np.diff(exp["point_offsets"][:3]).max()))
    assert torch.equal(mine["voxel_offsets"], theirs["voxel_offsets"])
    total = int(mine["voxel_offsets"][-1])
    assert total > 500
    assert torch.equal(mine["voxel_coords"][:total], theirs["voxel_coords"][:total])
    assert torch.equal(mine["voxel_num_points"][:total], theirs["voxel_num_points"][:total])
    from lidardetection_amd.pointpillar import PointPillarKITTI
    torch.manual_seed(0)
    model = PointPillarKITTI(batch_size=2, device=DEV).train()
    losses = model.train_loss(out["points"], out["point_offsets"], out["gt_boxes"])
    assert len(losses) == 3 and all(bool(torch.isfinite(v)) for v in losses)
