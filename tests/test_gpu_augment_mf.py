"""GPU checks of the multi-frame poses through the train-time augmentation (lidar_augment_mf in csrc/augment.hip, through
lidardetection_amd/augment.py and the raw C ABI): every case of tests/golden/augment_mf_ref.npz (written by the reference itself), the
shared outputs bitwise against the plain lidar_augment call, edge shapes against the numpy restatement (tests/_augment_mf_np.py) with
inputs drawn under the golden file's borderline condition, the zero padding, reproducibility, graph capture, the refusals, and the
path into the consumers of the poses (point_head_mf).  Counts, offsets, sample_valid and row orders compare exactly; coordinates, boxes
and poses to the project's stated 1e-4, |a - b| <= 1e-4 * max(1, |b|)."""
import numpy as np
import pytest
import torch

import _augment_mf_np as amf
import _augment_np as anp
import _point_head_mf_np as mf
from test_point_head_mf_host import make_head
from lidardetection_amd import _lib, augment, point_head_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHARED = ("points", "point_offsets", "gt_boxes", "gt_counts", "sample_valid")


def _up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _augmentor(inp, cfg, poses=True):
    pose = dict(locations=inp["db_locations"], rotations_y=inp["db_rotations_y"]) if poses else {}
    db = augment.GtDatabase(inp["db_points"], inp["db_offsets"], inp["db_boxes"], inp["db_cls"], device=DEV, **pose)
    aug = augment.TrainAugmentor(db, inp["cand"].shape[1], cfg["pc_range"], remove_extra_width=cfg["remove_extra_width"],
                                 collide_extra_width=cfg.get("collide_extra_width"), remove_outside_boxes=cfg["remove_outside_boxes"],
                                 min_num_corners=cfg["min_num_corners"], sample_rot_range=(0, 0) if "sample_rot" in inp else None)
    aug.apply_scale = cfg["apply_scale"]
    return aug


def _run(inp, cfg, poses=True, aug=None):
    aug = aug or _augmentor(inp, cfg, poses)
    pose = dict(locations=_up(inp["locations"], np.float32), rotations_y=_up(inp["rotations_y"], np.float32)) if poses else {}
    return aug(_up(inp["points"], np.float32), _up(inp["point_offsets"], np.int32), _up(inp["gt_boxes"], np.float32),
               _up(inp["gt_counts"], np.int32), inp["cand"], planes=inp.get("plane"), flip_x=inp["flip_x"], flip_y=inp["flip_y"],
               rot=inp["rot"], scale=inp["scale"], sample_rot=inp.get("sample_rot"), **pose)


def _host(out):
    offs = out["point_offsets"].cpu().numpy()
    got = {k: out[k].cpu().numpy() for k in out if torch.is_tensor(out[k])}
    got["points"] = got["points"][:int(offs[-1])]
    return got


def _compare(got, exp):
    for k in ("point_offsets", "gt_counts", "sample_valid"):
        print(k, got[k].reshape(-1)[:24], exp[k].reshape(-1)[:24])
        assert np.array_equal(got[k], exp[k]), k
    print("max |d points|", np.abs(got["points"] - exp["points"]).max(initial=0), "max |d boxes|", np.abs(got["gt_boxes"] - exp["gt_boxes"]).max(initial=0),
          "max |d locations|", np.abs(got["locations"] - exp["locations"]).max(initial=0),
          "max |d rotations_y|", np.abs(got["rotations_y"] - exp["rotations_y"]).max(initial=0))
    assert anp.close(got["points"], exp["points"]) and anp.close(got["gt_boxes"], exp["gt_boxes"])
    assert np.array_equal(got["points"][:, 3:], exp["points"][:, 3:])                # kept-row order: the features are copied bits
    assert np.array_equal(got["gt_boxes"][..., 7], exp["gt_boxes"][..., 7])          # box row order and the zero padding
    assert amf.pose_close(got, exp)
    for b, n in enumerate(exp["gt_counts"]):                                          # exact zeros at and past the count
        assert not got["locations"][b, n:].any() and not got["rotations_y"][b, n:].any()


class Raw:
    """the raw lidar_augment_mf / lidar_augment call on device copies of `inp`, outputs pre-filled with `fill`"""

    def __init__(self, inp, cfg, fill=float("nan")):
        self.L, self.inp, self.cfg = _lib.lib(), inp, cfg
        B, G, P = inp["cand"].shape
        self.B, self.G, self.P = B, G, P
        self.M, self.C, self.n = inp["gt_boxes"].shape[1], inp["points"].shape[1], inp["points"].shape[0]
        self.F = inp["locations"].shape[2]
        sizes = np.diff(inp["db_offsets"])
        self.n_obj = len(sizes)
        self.bound = int(np.where(inp["cand"] >= 0, sizes[np.maximum(inp["cand"], 0)], 0).sum()) if inp["cand"].size else 0
        self.cap = self.n + self.bound + 5
        rot64 = inp["rot"].astype(np.float64)
        f32, i32 = np.float32, np.int32
        self.d = {k: _up(inp.get(k), t) for k, t in (
            ("points", f32), ("point_offsets", i32), ("gt_boxes", f32), ("gt_counts", i32), ("db_points", f32), ("db_offsets", i32),
            ("db_boxes", f32), ("db_cls", i32), ("cand", i32), ("flip_x", i32), ("flip_y", i32), ("rot", f32), ("sample_rot", f32),
            ("plane", f32), ("locations", f32), ("rotations_y", f32), ("db_locations", f32), ("db_rotations_y", f32))}
        self.d["scale"] = _up(inp["scale"], f32) if cfg["apply_scale"] else None
        self.d["cs"] = _up(np.stack([np.cos(rot64), np.sin(rot64)], 1), f32)
        T = G * P
        self.o = dict(points=torch.full((self.cap, self.C), fill, device=DEV), point_offsets=torch.full((B + 1,), -7, dtype=torch.int32, device=DEV),
                      gt_boxes=torch.full((B, self.M + T, 8), fill, device=DEV), gt_counts=torch.full((B,), -7, dtype=torch.int32, device=DEV),
                      sample_valid=torch.full((B, G, P), -7, dtype=torch.int32, device=DEV),
                      locations=torch.full((B, self.M + T, self.F, 3), fill, device=DEV),
                      rotations_y=torch.full((B, self.M + T, self.F), fill, device=DEV))
        self.ws = torch.empty(max(int(self.L.lidar_augment_workspace_bytes(B, G, P, self.cap)), 1), dtype=torch.uint8, device=DEV)

    def _head(self):
        d, cfg, p = self.d, self.cfg, _lib.ptr
        cw = cfg.get("collide_extra_width")
        return (p(d["points"]), p(d["point_offsets"]), self.n, self.C, p(d["gt_boxes"]), p(d["gt_counts"]), self.B, self.M, p(d["db_points"]),
                p(d["db_offsets"]), p(d["db_boxes"]), p(d["db_cls"]), self.n_obj, int(self.inp["db_points"].shape[0]), p(d["cand"]), self.G,
                self.P, p(d["flip_x"]), p(d["flip_y"]), p(d["rot"]), p(d["cs"]), p(d["scale"]), p(d["sample_rot"]), p(d["plane"]),
                _lib.host_f32(cfg["remove_extra_width"]), None if cw is None else _lib.host_f32(cw), _lib.host_f32(cfg["pc_range"]),
                int(cfg["remove_outside_boxes"]), cfg["min_num_corners"], self.bound, self.cap)

    def _outs(self):
        o, p = self.o, _lib.ptr
        return p(o["points"]), p(o["point_offsets"]), p(o["gt_boxes"]), p(o["gt_counts"]), p(o["sample_valid"])

    def mf(self, frames=None, null=()):
        d, o, p = self.d, self.o, _lib.ptr
        pose = {k: None if k in null else v for k, v in (("locations", d["locations"]), ("rotations_y", d["rotations_y"]),
                                                         ("db_locations", d["db_locations"]), ("db_rotations_y", d["db_rotations_y"]),
                                                         ("out_locations", o["locations"]), ("out_rotations_y", o["rotations_y"]))}
        return self.L.lidar_augment_mf(*self._head(), p(pose["locations"]), p(pose["rotations_y"]), p(pose["db_locations"]),
                                       p(pose["db_rotations_y"]), self.F if frames is None else frames, *self._outs(),
                                       p(pose["out_locations"]), p(pose["out_rotations_y"]), p(self.ws), self.ws.numel(), _lib.stream())

    def plain(self):
        return self.L.lidar_augment(*self._head(), *self._outs(), _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def untouched(self):
        return all(bool(torch.isnan(v).all()) if v.is_floating_point() else bool((v == -7).all()) for v in self.o.values())


@pytest.mark.parametrize("name", amf.CASES)
def test_golden_through_train_augmentor(name):
    cfg, inp, exp, _ = amf.load_contract(name)
    out = _run(inp, cfg)
    B, M, F = inp["locations"].shape[:3]
    T = inp["cand"].shape[1] * inp["cand"].shape[2]
    assert tuple(out["locations"].shape) == (B, M + T, F, 3) and tuple(out["rotations_y"].shape) == (B, M + T, F)
    _compare(_host(out), exp)


def test_golden_through_the_c_abi():
    cfg, inp, exp, _ = amf.load_contract("plane3")
    raw = Raw(inp, cfg)
    assert raw.mf() == 0
    got = _host(raw.o)
    _compare(got, exp)
    assert bool(torch.isnan(raw.o["points"][int(got["point_offsets"][-1]):]).all())   # nothing is written past the last row


@pytest.mark.parametrize("name", amf.CASES)
def test_shared_outputs_are_bitwise_those_of_the_plain_call(name):
    cfg, inp, exp, _ = amf.load_contract(name)
    with_p, without = _host(_run(inp, cfg)), _host(_run(inp, cfg, poses=False))
    assert sorted(without) == sorted(SHARED) and sorted(with_p) == sorted(SHARED + ("locations", "rotations_y"))
    for k in SHARED:
        assert np.array_equal(with_p[k].view(np.int32), without[k].view(np.int32)), k
    a, b = Raw(inp, cfg, fill=0.0), Raw(inp, cfg, fill=0.0)                           # and through the raw ABI, whole buffers
    assert a.mf() == 0 and b.plain() == 0
    for k in SHARED:
        assert torch.equal(a.o[k].view(torch.int32), b.o[k].view(torch.int32)), k


EDGE = {
    "class_id_0": dict(frame_points=[300, 257, 100], frames=3),                       # every second annotation is untrained
    "no_annotations": dict(frame_points=[300, 200], n_gt=0, frames=2),
    "per_group_0": dict(frame_points=[300, 200], S=0, frames=3),
    "plain": dict(frame_points=[400, 300, 200], plane=False, sample_rot=False, collide=False, scale=False, frames=3),
    "no_scale": dict(frame_points=[300, 200], scale=False, frames=1),
    "no_plane": dict(frame_points=[300, 200], plane=False, frames=8),
    "no_sample_rot": dict(frame_points=[300, 200], sample_rot=False, frames=2),
    "boxes_512": dict(frame_points=[200, 100], M=8, G=8, S=63, n_db=144, n_gt=8, frames=3),
    "all_dropped": dict(frame_points=[300, 200], frames=3, drop_frame=0),
}


def _edge_inputs(name):
    spec = dict(EDGE[name])
    frames, drop = spec.pop("frames"), spec.pop("drop_frame", None)
    for seed in range(sum(map(ord, name)), sum(map(ord, name)) + 50):
        inp, cfg = anp.synth_inputs(seed, **spec)
        if drop is not None:                  # flip y negates x, and no rotation: no box of the frame keeps a corner inside x >= 0
            inp["flip_y"][drop] = 1
            inp["rot"][drop] = 0.0
        inp = amf.add_poses(inp, frames, seed)
        if drop is None or amf.borderline_clear(inp, cfg):
            return inp, cfg
    raise RuntimeError("no seed keeps every decision clear of its threshold")


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes_against_the_restatement(name):
    inp, cfg = _edge_inputs(name)
    exp = amf.augment(inp, cfg)
    got = _host(_run(inp, cfg))
    _compare(got, exp)
    B, M = inp["gt_boxes"].shape[:2]
    if name == "class_id_0":
        real = [inp["gt_boxes"][b, :inp["gt_counts"][b], 7] for b in range(B)]
        assert any((r == 0).any() and (r > 0).any() for r in real)
    if name == "no_annotations":
        assert not inp["gt_counts"].any() and exp["gt_counts"].sum() > 0
    if name == "per_group_0":
        assert got["locations"].shape[1] == M and exp["gt_counts"].sum() > 0
    if name == "plain":
        assert "plane" not in inp and "sample_rot" not in inp and not cfg["apply_scale"] and cfg["collide_extra_width"] is None
    if name == "boxes_512":
        assert M + inp["cand"].shape[1] * inp["cand"].shape[2] == 512 and exp["sample_valid"].sum() > 100
    if name == "all_dropped":
        assert inp["gt_counts"][0] > 0 and exp["sample_valid"][0].sum() > 0 and exp["gt_counts"][0] == 0 and exp["gt_counts"][1] > 0
        assert not got["gt_boxes"][0].any() and not got["locations"][0].any() and not got["rotations_y"][0].any()


def test_every_pose_element_is_written_over_nan():
    inp, cfg = _edge_inputs("class_id_0")
    raw = Raw(inp, cfg)
    assert raw.mf() == 0
    got = _host(raw.o)
    assert np.isfinite(got["locations"]).all() and np.isfinite(got["rotations_y"]).all() and np.isfinite(got["gt_boxes"]).all()
    assert 0 < got["gt_counts"].min() and got["gt_counts"].max() < got["locations"].shape[1]
    for b, n in enumerate(got["gt_counts"]):
        assert not got["locations"][b, n:].any() and not got["rotations_y"][b, n:].any()
        assert got["locations"][b, :n].any(axis=(1, 2)).all()
    _compare(got, amf.augment(inp, cfg))


def test_two_calls_are_bitwise_identical_and_a_graph_replays_them():
    cfg, inp, exp, _ = amf.load_contract("plane3")
    aug = _augmentor(inp, cfg)
    a, b = _host(_run(inp, cfg, aug=aug)), _host(_run(inp, cfg, aug=aug))
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    # capture the raw call (the wrapper's uploads are not part of it), replay once
    raw = Raw(inp, cfg, fill=0.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert raw.mf() == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in raw.o.values():
        v.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status = raw.mf()
    assert status == 0
    graph.replay()
    torch.cuda.synchronize()
    c = _host(raw.o)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), c[k].view(np.int32)), k


def test_batch_of_zero_frames():
    inp, cfg = anp.synth_inputs(5, [10])
    inp = amf.add_poses(inp, 3)
    aug = _augmentor(inp, cfg)
    out = aug(torch.zeros((0, 4), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros((0, 8, 8), device=DEV),
              torch.zeros(0, dtype=torch.int32, device=DEV), np.zeros((0, 3, 15), np.int32), flip_x=np.zeros(0), flip_y=np.zeros(0),
              rot=np.zeros(0), scale=np.zeros(0), sample_rot=np.zeros((0, 3, 15)), locations=torch.zeros((0, 8, 3, 3), device=DEV),
              rotations_y=torch.zeros((0, 8, 3), device=DEV))
    assert out["points"].shape == (0, 4) and out["point_offsets"].tolist() == [0]
    assert out["locations"].shape == (0, 8 + 45, 3, 3) and out["rotations_y"].shape == (0, 8 + 45, 3)
    raw = Raw(inp, cfg)                       # the raw call with batch 0: status 0 and no launch, so nothing is written
    raw.B = 0
    assert raw.mf() == 0
    torch.cuda.synchronize()
    assert raw.untouched()


def test_refusals_leave_the_outputs_untouched():
    cfg, inp, exp, _ = amf.load_contract("yaml3")
    raw = Raw(inp, cfg)
    for null in ("locations", "rotations_y", "db_locations", "db_rotations_y", "out_locations", "out_rotations_y"):
        assert raw.mf(null=(null,)) == -1, null
    assert raw.mf(frames=9) == -1 and raw.mf(frames=0) == -1
    aligned = raw.d["locations"]
    raw.d["locations"] = aligned.view(torch.uint8).flatten()[1:]                      # misaligned by one byte
    assert raw.d["locations"].data_ptr() == aligned.data_ptr() + 1 and raw.mf() == -1
    torch.cuda.synchronize()
    assert raw.untouched()


def test_into_the_consumers_of_the_poses():
    """the layout contract between lidar_augment_mf and point_head_mf: zero-padded rows, counts, column order.  The device functions on
    the call's outputs against the mirror head's torch formulation on the same tensors copied to the host (labels and owners exactly);
    the union boxes, which have no torch formulation in the package, against the float64 restatement the point-head tests pin to the
    reference (1e-4).  The points keep 1e-3 clear of every face of every per-sweep box, so that no label hangs on a rounding."""
    cfg, inp, exp, _ = amf.load_contract("yaml3")
    out = _run(inp, cfg)
    gt, loc, rot = out["gt_boxes"], out["locations"], out["rotations_y"]
    g, l, r = (t.cpu().numpy() for t in (gt, loc, rot))
    counts = out["gt_counts"].cpu().numpy()
    rs = np.random.default_rng(21)
    pts = []
    for b, n in enumerate(counts):
        if n:
            k, s = rs.integers(0, n, 300), rs.integers(0, l.shape[2], 300)
            near = l[b, k, s] + rs.normal(0, 1, (300, 3)) * g[b, k, 3:6] * 0.5
            pts.append(np.concatenate([np.full((300, 1), b), near], 1))
        pts.append(np.concatenate([np.full((100, 1), b), rs.uniform([0, -40, -3], [70, 40, 1], (100, 3))], 1))
    pts = np.concatenate(pts, 0).astype(np.float32)
    pts = pts[mf.margins_mf(pts, g, l, r, mf.EXTRA) >= 1e-3]
    head = make_head("classes2", stack_frame_size=int(l.shape[2]))
    spec = head.fused_spec()
    assert spec is not None and point_head_mf.supported(len(pts), *g.shape[:2], l.shape[2], 2)
    dev = point_head_mf.assign_point_targets_mf(_up(pts), gt, loc, rot, spec)
    cpu = head._assign({"point_coords": torch.from_numpy(pts), "gt_boxes": gt.cpu(), "locations": loc.cpu(), "rotations_y": rot.cpu()})
    labels = dev["point_cls_labels_stacked"].cpu()
    assert torch.equal(labels, cpu["point_cls_labels_stacked"]) and torch.equal(dev["point_box_idx"].cpu(), cpu["point_box_idx"])
    assert int((labels > 0).sum()) > 100 and int((labels == 2).sum()) > 0 and int((labels < 0).sum()) > 0
    owner = dev["point_box_idx"].cpu().numpy()
    assert (owner < counts[pts[:, 0].astype(int)][:, None]).all()                     # no point is owned by a padding row
    enl = point_head_mf.enlarged_gt_boxes(gt, loc, rot).cpu().numpy()
    ref = mf.enlarged(g, l)
    print("union boxes from the augmented poses: max err", np.abs(enl - ref).max())
    assert anp.close(enl, ref)
    for b, n in enumerate(counts):
        assert not enl[b, n:].any() and (enl[b, :n, 3:5] >= g[b, :n, 3:5] - 1e-4).all()
