"""Generates tests/golden/atss_assign_ref.npz from the REFERENCE ITSELF: its own ATSSTargetAssigner
(pcdet/models/dense_heads/target_assigner/atss_target_assigner.py), AnchorGenerator (anchor_generator.py) and ResidualCoder
(pcdet/utils/box_coder_utils.py), loaded stand-alone from their files and run on the CPU.  Runs only where the reference checkout
is (default /root/reference, or $LIDAR_REFERENCE) and oracle/_ref is built; the .npz (inputs, anchors, the IoU matrices the
reference saw, outputs) is what the tests read.

The CUDA wrapper iou3d_nms_utils.boxes_iou_bev is replaced by the reference's own compiled boxes_iou_bev_cpu (oracle/_ref through
oracle/ref_loader.py).  For match_height the 3D IoU is RESTATED here in numpy from that BEV IoU (overlap recovered from the IoU,
times the height overlap, over the union volume): the case is marked `restated_iou3d` in its meta.  torch.Tensor.cuda is the
identity while the reference runs.

Reference anchor grids put two rotations on one centre, so the TOPK-th distance would always be tied; the anchors (an input) are
jittered per rotation by a fixed small offset.

Decision margins, ASSERTED for every recorded case so that fp32 reordering on the device cannot flip an outcome:
  each gt's TOPK-th vs (TOPK+1)-th distance      differ by more than 1e-5 relative
  every candidate IoU vs its gt's threshold      more than 1e-3 away   (*)
  each gt's best vs second-best IoU over a set   differ by more than 1e-3, unless both are exactly 0
  per anchor, its two best positive gts          differ by more than 1e-3
  every candidate's centre-in-box comparisons    more than 1e-4 away (ours, not the issue's)
(*) a gt whose candidates' IoUs are ALL exactly 0 (outside the range, an all-zero row, a gt between small anchors) has the
threshold 1e-6 exactly, in the reference and on the device alike (a rejected pair is exactly 0 on both); the cases the fixture
must hold need such gts, so they are exempt, like the exact-zero exemption of the third row.
Every drawn gt (the random ones, and the special ones whose position or size is drawn) is drawn again until the frame with it meets
every margin; the fixed rows (the all-zero row, the out-of-range gt) must meet them as they are.  Nothing is excluded afterwards.

Cases
  kitti     3 sets (Car, Pedestrian, Cyclist anchors), single head, TOPK 9, B 3, M 12: a frame of only padding; a trailing row
            that sums to 0 without being zero; an interior all-zero row; a gt outside the anchor range (forces anchor 0) AFTER
            the all-zero row, so two gts force anchor 0 and the later one must win; a class-0 gt and a negative-class gt; a gt
            whose candidates all fail the centre-in-box test
  kitti_k2  TOPK 2, and a second set of exactly 2 anchors (n_k == TOPK)
  nus       use_multihead, ResidualCoder(code_size=9, encode_angle_by_sincos=True), 9-column gts, anchors zero-padded to 9
  kitti_3d  the kitti inputs with match_height True (restated 3D IoU)

Usage:  python tests/golden/make_atss_golden.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refpcdet_atss"

import _atss_np as atn  # noqa: E402
from oracle import ref_loader  # noqa: E402

RECORD = []   # the IoU matrices the reference computed, in call order (set-major, then frame)


def ref_iou_bev(a, b):
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32)
    ref_loader.load("iou3d_nms_cuda").boxes_iou_bev_cpu(a.contiguous().float(), b.contiguous().float(), out)
    return out


def stub_iou_bev(a, b):
    out = ref_iou_bev(a, b)
    RECORD.append(out.numpy().copy())
    return out


def stub_iou3d(a, b):
    an, bn = a.numpy(), b.numpy()
    iou = atn.iou3d_from_bev_overlap(atn.bev_overlap_from_iou(ref_iou_bev(a, b).numpy(), an, bn), an, bn)
    RECORD.append(iou.copy())
    return torch.from_numpy(iou)


def load_reference():
    """-> (atss_target_assigner, anchor_generator, box_coder_utils) modules of the reference"""
    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    root = os.path.join(REF, "pcdet")
    for sub in ["", ".utils", ".ops", ".ops.iou3d_nms", ".ops.roiaware_pool3d", ".models", ".models.dense_heads",
                ".models.dense_heads.target_assigner"]:
        pkg(PKG + sub, os.path.join(root, *sub.split(".")[1:]))
    sys.modules.setdefault("quaternion", types.ModuleType("quaternion"))
    iou_stub = types.ModuleType(PKG + ".ops.iou3d_nms.iou3d_nms_utils")
    iou_stub.boxes_iou_bev, iou_stub.boxes_iou3d_gpu = stub_iou_bev, stub_iou3d
    sys.modules[iou_stub.__name__] = iou_stub
    sys.modules[PKG + ".ops.iou3d_nms"].iou3d_nms_utils = iou_stub
    roi_stub = types.ModuleType(PKG + ".ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules[roi_stub.__name__] = roi_stub
    sys.modules[PKG + ".utils"].common_utils = load(PKG + ".utils.common_utils", os.path.join(root, "utils", "common_utils.py"))
    load(PKG + ".utils.box_utils", os.path.join(root, "utils", "box_utils.py"))
    coder = load(PKG + ".utils.box_coder_utils", os.path.join(root, "utils", "box_coder_utils.py"))
    ta = os.path.join(root, "models", "dense_heads", "target_assigner")
    gen = load(PKG + ".models.dense_heads.target_assigner.anchor_generator", os.path.join(ta, "anchor_generator.py"))
    asg = load(PKG + ".models.dense_heads.target_assigner.atss_target_assigner", os.path.join(ta, "atss_target_assigner.py"))
    return asg, gen, coder


GRID = [12, 10]
KITTI_RANGE = [0.0, -7.2, -3, 17.6, 7.2, 1]          # stride 1.6 both ways on the 12 x 10 map
KITTI_CFG = [
    dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
         align_center=False, feature_map_stride=2),
    dict(class_name="Pedestrian", anchor_sizes=[[0.8, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
         align_center=False, feature_map_stride=2),
    dict(class_name="Cyclist", anchor_sizes=[[1.76, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
         align_center=False, feature_map_stride=2),
]
NUS_RANGE = [-8.8, -7.2, -5.0, 8.8, 7.2, 3.0]
NUS_CFG = [
    dict(class_name="car", anchor_sizes=[[4.63, 1.97, 1.74]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.95],
         align_center=False, feature_map_stride=4),
    dict(class_name="truck", anchor_sizes=[[6.93, 2.51, 2.84]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
         align_center=False, feature_map_stride=4),
    dict(class_name="motorcycle", anchor_sizes=[[2.11, 0.77, 1.47]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.085],
         align_center=False, feature_map_stride=4),
]
JITTER = [(0.013, -0.007), (-0.011, 0.009)]    # per rotation, metres


def make_anchors(gen, cfg, pc_range, ndim=7):
    anchors, _ = gen.AnchorGenerator(anchor_range=pc_range, anchor_generator_config=cfg).generate_anchors([GRID] * len(cfg))
    out = []
    for a in anchors:
        a = a.clone()
        for r, (jx, jy) in enumerate(JITTER):
            a[..., r, 0] += jx
            a[..., r, 1] += jy
        if ndim > 7:
            a = torch.cat((a, a.new_zeros([*a.shape[:-1], ndim - 7])), dim=-1)
        out.append(a)
    return out


def flatten(anchors, multihead):
    return [(a.permute(3, 4, 0, 1, 2, 5) if multihead else a).contiguous().view(-1, a.shape[-1]).numpy() for a in anchors]


def frame_problems(flat, gts, topk, iou_fn):
    """margin violations of one frame's (trimmed) gt boxes against every set -> list of strings"""
    bad = []
    for k, a in enumerate(flat):
        ious = iou_fn(a[:, :7], gts[:, :7])
        dist = atn.distances(a, gts).astype(np.float64)
        n = a.shape[0]
        positive = {}
        for j in range(gts.shape[0]):
            order = np.lexsort((np.arange(n), dist[:, j]))
            if n > topk:
                d0, d1 = dist[order[topk - 1], j], dist[order[topk], j]
                if not (d1 - d0) > 1e-5 * max(d1, 1e-12):
                    bad.append(f"set {k} gt {j}: distance tie {d0} {d1}")
            cand = order[:topk]
            ci = ious[cand, j].astype(np.float64)
            thr = ci.mean() + ci.std(ddof=1) + 1e-6
            if not (ci == 0).all() and np.abs(ci - thr).min() <= 1e-3:
                bad.append(f"set {k} gt {j}: candidate IoU within 1e-3 of the threshold {thr}")
            col = np.sort(ious[:, j].astype(np.float64))[::-1]
            if n > 1 and not (col[0] == 0 and col[1] == 0) and col[0] - col[1] <= 1e-3:
                bad.append(f"set {k} gt {j}: best two IoUs {col[0]} {col[1]}")
            g = gts[j].astype(np.float64)
            lx, ly = a[cand, 0] - g[0], a[cand, 1] - g[1]
            rx, ry = lx * np.cos(g[6]) + ly * np.sin(g[6]), -lx * np.sin(g[6]) + ly * np.cos(g[6])
            if min(np.abs(np.abs(rx) - g[4] / 2).min(), np.abs(np.abs(ry) - g[3] / 2).min()) <= 1e-4:
                bad.append(f"set {k} gt {j}: centre on the box edge")
            inside = (np.abs(rx) <= g[4] / 2) & (np.abs(ry) <= g[3] / 2)
            for c, v in zip(cand[(ci >= thr) & inside], ci[(ci >= thr) & inside]):
                positive.setdefault(int(c), []).append(v)
        for c, vals in positive.items():
            vals = sorted(vals, reverse=True)
            if len(vals) > 1 and vals[0] - vals[1] <= 1e-3:
                bad.append(f"set {k} anchor {c}: two positive gts {vals[0]} {vals[1]}")
    return bad


def sample_frame(rng, flat, specs, topk, iou_fn):
    """one frame's rows from `specs`: a fixed row (must meet the margins as it is) or a callable(rng) drawn again until the frame
    with it still meets every margin"""
    rows = []
    for spec in specs:
        for tries in range(3000):
            row = np.asarray(spec(rng) if callable(spec) else spec, np.float32)
            problems = [q for fn in (iou_fn if isinstance(iou_fn, (list, tuple)) else [iou_fn])
                        for q in frame_problems(flat, np.stack(rows + [row])[:, :-1], topk, fn)]
            if not problems:
                rows.append(row)
                break
            assert callable(spec), problems
        else:
            raise AssertionError(f"no gt meets the margins: {problems}")
    return rows


def kitti_draw(rng):
    c = int(rng.integers(1, 4))
    size = np.array(KITTI_CFG[c - 1]["anchor_sizes"][0]) * rng.uniform(0.85, 1.15, 3)
    return [rng.uniform(1, 16.5), rng.uniform(-6.5, 6.5), rng.uniform(-1.2, -0.4), *size, rng.uniform(-np.pi, np.pi), c]


def nus_draw(rng):
    c = int(rng.integers(1, 4))
    size = np.array(NUS_CFG[c - 1]["anchor_sizes"][0]) * rng.uniform(0.85, 1.15, 3)
    return [rng.uniform(-8, 8), rng.uniform(-6.5, 6.5), rng.uniform(-1.5, 0.5), *size, rng.uniform(-np.pi, np.pi),
            *rng.normal(0, 3, 2), c]


def kitti_gt(flat, topk, iou_fn, seed, M=12):
    rng = np.random.default_rng(seed)
    gt = np.zeros((3, M, 8), np.float32)
    # frame 0: a gt in the middle of a cell (every candidate's centre is outside it), a class-0 gt, a negative-class gt, an
    # interior all-zero row, then a gt outside the range (anchor 0 is forced by both; the later one wins), random gts, and a
    # trailing row that sums to 0 without being zero
    def between(r):       # thin, in the middle of a cell: 0.8 m from the nearest anchor centres either way
        return [8.8 + r.uniform(-0.05, 0.05), 0.8 + r.uniform(-0.05, 0.05), -0.6, r.uniform(2.2, 2.8), r.uniform(0.7, 1.0), 1.73,
                r.uniform(-0.08, 0.08), 2]

    def with_class(c):
        return lambda r: [*kitti_draw(r)[:-1], c]

    special = [between, with_class(0), with_class(-1), [0, 0, 0, 0, 0, 0, 0, 0], [30.0, 21.0, -1.0, 3.9, 1.6, 1.56, 0.3, 2]]
    rows = sample_frame(rng, flat, special + [kitti_draw] * 4, topk, iou_fn)
    rows.append(np.array([1.0, -1.0, 0, 0, 0, 0, 0, 2], np.float32))
    gt[0, :len(rows)] = np.stack(rows)
    # frame 1: only padding.  frame 2: random gts filling every row
    gt[2] = np.stack(sample_frame(rng, flat, [kitti_draw] * M, topk, iou_fn))
    return gt


def check_special(flat, gt, topk, iou_fn):
    """the kitti special rows do what the docstring says"""
    g = gt[0, :atn.trim_count(gt[0, :, :-1]), :-1]
    assert g.shape[0] == 9 and gt[0, 9, :2].tolist() == [1.0, -1.0], "the trailing row must be trimmed"
    some_pos = False
    for a in flat:
        ious = iou_fn(a[:, :7], g[:, :7])
        assert ious[:, 3].max() == 0 and ious[:, 4].max() == 0, "the zero row and the outside gt overlap nothing"
        cand = atn.topk_candidates(atn.distances(a, g)[:, 0], topk)
        assert not atn.centre_inside(a[cand], g[0]).any(), "a candidate's centre is inside the in-between gt"
        ci = ious[cand, 0]
        some_pos |= bool((ci >= atn.threshold(ci.astype(np.float32))).any())
    assert some_pos, "the in-between gt has no candidate above its threshold in any set"


def run_case(asg, coder, name, anchors, gt, topk, multihead=False, match_height=False, code_size=7, sincos=False, out=None):
    box_coder = coder.ResidualCoder(code_size=code_size, encode_angle_by_sincos=sincos)
    del RECORD[:]
    res = asg.ATSSTargetAssigner(topk, box_coder, match_height=match_height).assign_targets(
        list(anchors), torch.from_numpy(gt), use_multihead=multihead)
    meta = dict(topk=topk, use_multihead=multihead, match_height=match_height, code_size=box_coder.code_size,
                encode_angle_by_sincos=sincos, num_anchors=len(anchors), restated_iou3d=bool(match_height))
    out[f"{name}_meta"] = np.array(json.dumps(meta))
    out[f"{name}_gt"] = gt
    for k, t in enumerate(anchors):
        out[f"{name}_anchors_{k}"] = t.numpy()
    it = iter(RECORD)
    for k in range(len(anchors)):
        for b in range(gt.shape[0]):
            out[f"{name}_iou_{b}_{k}"] = next(it)
    out[f"{name}_labels"] = res["box_cls_labels"].numpy()
    out[f"{name}_targets"] = res["box_reg_targets"].numpy()
    out[f"{name}_weights"] = res["reg_weights"].numpy()
    lab = res["box_cls_labels"]
    print(name, tuple(lab.shape), "pos", int((lab > 0).sum()), "zero", int((lab == 0).sum()), "neg", int((lab < 0).sum()))


def main():
    assert ref_loader.load("iou3d_nms_cuda") is not None, "oracle/_ref is not built (oracle/build_ref.py)"
    asg, gen, coder = load_reference()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    bev = lambda a, g: ref_iou_bev(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(g))).numpy()  # noqa: E731
    iou3d = lambda a, g: atn.iou3d_from_bev_overlap(atn.bev_overlap_from_iou(bev(a, g), a, g), a, g)  # noqa: E731
    try:
        anchors = make_anchors(gen, KITTI_CFG, KITTI_RANGE)
        flat = flatten(anchors, False)
        # one gt tensor serves kitti and kitti_3d: every row is drawn until both IoUs meet the margins
        gt = kitti_gt(flat, 9, [bev, iou3d], 21)
        check_special(flat, gt, 9, bev)
        run_case(asg, coder, "kitti", anchors, gt, 9, out=out)
        run_case(asg, coder, "kitti_3d", anchors, gt, 9, match_height=True, out=out)

        # TOPK 2; the second set is exactly two anchors
        two = anchors[2][0:1, 4:5, 6:7].clone()       # (1, 1, 1, 1, 2, 7)
        sets2 = [anchors[0], two]
        flat2 = flatten(sets2, False)
        rng = np.random.default_rng(33)
        gt2 = np.zeros((3, 6, 8), np.float32)
        for b, n in enumerate([6, 3, 1]):
            gt2[b, :n] = np.stack(sample_frame(rng, flat2, [kitti_draw] * n, 2, bev))
        run_case(asg, coder, "kitti_k2", sets2, gt2, 2, out=out)

        nanchors = make_anchors(gen, NUS_CFG, NUS_RANGE, ndim=9)
        nflat = flatten(nanchors, True)
        rng = np.random.default_rng(44)
        ngt = np.zeros((3, 10, 10), np.float32)
        for b, n in enumerate([10, 5, 7]):
            ngt[b, :n] = np.stack(sample_frame(rng, nflat, [nus_draw] * n, 9, bev))
        run_case(asg, coder, "nus", nanchors, ngt, 9, multihead=True, code_size=9, sincos=True, out=out)
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "atss_assign_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
