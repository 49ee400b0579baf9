"""Generates tests/golden/point_head_mf_ref.npz from the REFERENCE ITSELF: its own PointHeadSimpleMultiFrame (assign_targets,
get_loss) and the literal lines 67-88 of its AnchorHeadSingle.forward (the USE_MULTIFRAME_ENLARGED_GT_BOXES block), read from the
reference's file at run time and executed on the CPU.  Runs only where the reference checkout is ($LIDAR_REFERENCE, or the
default of make_point_head_golden.py); the .npz is what the tests read.  The method, the module loader and the shims are
tests/golden/make_point_head_golden.py's: modules loaded standalone from their files, points_in_boxes_gpu stubbed by
oracle.c_oracle.points_in_boxes_gpu (which also records the owners), torch.Tensor.cuda the identity, and a float32 and a float64
run (torch.Tensor.float is .double() while the latter is on), both under autograd.

Stored per case <c> of tests/_point_head_mf_np.py:CASES: <c>_points (N, 4), <c>_gt (B, M, 8), <c>_loc (B, M, S, 3), <c>_rot
(B, M, S), <c>_labels (N, S) int64, <c>_owner (N, S) int32, <c>_pred_cls (N, S * num_class) int16 on the 1/64 grid, <c>_loss{32,64}
(the weighted cls term), <c>_pos, <c>_tb{32,64} (the tb_dict as JSON), <c>_gcls{32,64} (the gradient of the loss the head returns),
<c>_planted (rows of the planted points: moving, always ignored, origin).  Union boxes: enl_gt (3, 6, 8), enl_loc (3, 6, 3, 3),
enl_rot (3, 6, 3), enl32 / enl64 (3, 6, 8).  `cases`: CASES as JSON.

Scene (B 3, M 6): entry 0 has two overlapping gts first (they move together; a planted point in the overlap: the first wins), a gt
that moves so that one planted point at its frame-0 centre is foreground in frame 0, in the shell only in frame 1 and background in
frame 2, a gt that stands still with a planted point in its shell (ignored in every frame), and two padding rows with zero poses
that own the planted origin point; entry 1 has no padding; entry 2 has gts and no points; one row has bs_idx == B; headings lie up
to two turns outside [-pi, pi]; the rows are shuffled.  Logits include exactly 0 and +-20.

Asserted on the reference's numbers alone, moving to the next seed otherwise: apart from the planted origin point (named `origin`
below: every operand of its test against a padding row is exactly 0) no point lies within 1e-4 of a face of any per-frame box or
enlarged box (tests/_point_head_mf_np.py:margins_mf); the generator also asserts that the reference's union boxes do not change
when rotations_y does.

Usage:  python tests/golden/make_point_head_mf_golden.py
"""
import importlib.util
import json
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_point_head_golden as base  # noqa: E402
import _point_head_mf_np as mf  # noqa: E402
import _point_head_np as ph  # noqa: E402

B, M = 3, 6
ANCHOR_LINES = (67, 88)      # anchor_head_single.py, 1-based, inclusive


def load_reference():
    """-> the reference's PointHeadSimpleMultiFrame class and a function running lines 67-88 of AnchorHeadSingle.forward"""
    base.load_reference()
    d = os.path.join(base.REF, "pcdet", "models", "dense_heads")
    name = base.PKG + ".models.dense_heads.point_head_simple_multiframe"
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "point_head_simple_multiframe.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    with open(os.path.join(d, "anchor_head_single.py")) as fh:
        lines = fh.read().split("\n")[ANCHOR_LINES[0] - 1:ANCHOR_LINES[1]]
    code = compile(textwrap.dedent("\n".join(lines)), "anchor_head_single.py:%d-%d" % ANCHOR_LINES, "exec")
    env = {"torch": torch, "boxes_to_corners_3d": sys.modules[base.PKG + ".utils.box_utils"].boxes_to_corners_3d,
           "rotate_points_along_z": sys.modules[base.PKG + ".utils.common_utils"].rotate_points_along_z}

    def union_boxes(gt, loc, rot):
        scope = dict(env, data_dict={"gt_boxes": gt, "locations": loc, "rotations_y": rot})
        exec(code, scope)
        return scope["gt_boxes_enlarged"]
    return mod.PointHeadSimpleMultiFrame, union_boxes


def make_head(cls, case):
    h = cls.__new__(cls)
    nn.Module.__init__(h)
    h.model_cfg, h.num_class, h.stack_frame_size = base.to_cfg(case["cfg"]), case["num_class"], case["frames"]
    h.build_losses(h.model_cfg.LOSS_CONFIG)
    return h


def scene(seed, S, num_class):
    """-> points (N, 4), gt (B, M, 8), loc (B, M, S, 3), rot (B, M, S) float32, rows of the planted points"""
    r = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    for b, n in ((0, 4), (1, M), (2, 5)):
        gt[b, :n, 0:2] = r.uniform(-18, 18, (n, 2))
        gt[b, :n, 0:2] += np.sign(gt[b, :n, 0:2]) * 3        # nothing real near the origin
        gt[b, :n, 2] = r.uniform(-1.2, 0.2, n)
        k = r.integers(0, 3, n)
        gt[b, :n, 3:6] = np.asarray(ph.MEAN_SIZE, np.float32)[k] * r.uniform(0.85, 1.2, (n, 3))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n) + 2 * np.pi * r.integers(-2, 3, n)
        gt[b, :n, 7] = r.integers(1, num_class + 1, n)
    gt[0, 1] = gt[0, 0]
    gt[0, 1, 0:2] += [0.6, 0.3]                               # overlaps gt 0
    gt[0, 1, 6] += 0.4
    gt[0, 1, 7] = (gt[0, 0, 7] % num_class) + 1
    loc, rot = mf.moved_poses(r, gt, S, shift=0.5, turn=0.25)
    loc[0, 1] = loc[0, 0] + np.float32([0.6, 0.3, 0])         # the overlapping pair moves together
    rot[0, 1] = rot[0, 0] + np.float32(0.4)
    # gt (0, 2) keeps its heading and moves: 5 cm past the point along its own x axis in frame 1, 3 m away in frame 2
    g = gt[0, 2].astype(np.float64)
    ax = np.array([np.cos(g[6]), np.sin(g[6]), 0.0])
    for s, off in enumerate((0.0, g[3] / 2 + 0.05, 3.0 + g[3])[:S]):
        loc[0, 2, s], rot[0, 2, s] = g[0:3] - off * ax, g[6]
    loc[0, 3], rot[0, 3] = gt[0, 3, 0:3], gt[0, 3, 6]         # gt (0, 3) stands still
    g3 = gt[0, 3].astype(np.float64)
    c3, s3 = np.cos(g3[6]), np.sin(g3[6])
    l3 = np.array([g3[3] / 2 + 0.05, 0.1 * g3[4], 0.1 * g3[5]])
    planted = [[0, *g[0:3]],                                                            # moving: fg, shell, background
               [0, g3[0] + l3[0] * c3 - l3[1] * s3, g3[1] + l3[0] * s3 + l3[1] * c3, g3[2] + l3[2]],      # ignored in every frame
               [0, 0.0, 0.0, 0.0],                                                      # origin: owned by the first padding row
               [0, *((loc[0, 0, 0].astype(np.float64) + loc[0, 1, 0]) / 2)],            # in the overlap of gts 0 and 1 (frame 0)
               [0, 0.05, 0.03, 0.02],                                                   # ignored through the enlarged padding row
               [0, 60.0, 60.0, 5.0],                                                    # outside everything
               [B, 1.0, 1.0, 0.0]]                                                      # a bs_idx that names no entry
    pts = []
    for b, n in ((0, 150), (1, 140)):
        real = np.nonzero(gt[b, :, 3] > 0)[0]
        bg = np.stack([np.full(n // 3, b), r.uniform(-22, 22, n // 3), r.uniform(-22, 22, n // 3), r.uniform(-2.5, 1.5, n // 3)], 1)
        k, s = r.choice(real, n - n // 3), r.integers(0, S, n - n // 3)
        xyz = loc[b, k, s].astype(np.float64) + r.normal(0, 1, (len(k), 3)) * gt[b, k, 3:6] * 0.5
        pts += [bg, np.concatenate([np.full((len(k), 1), b), xyz], 1)]
    pts = np.concatenate(pts + [np.asarray(planted, np.float64)]).astype(np.float32)
    pts = pts[r.permutation(len(pts))]

    def row(p):
        hit = np.nonzero((pts == np.asarray(p, np.float64).astype(np.float32)).all(axis=1))[0]
        assert len(hit) == 1
        return int(hit[0])
    return pts, gt, loc, rot, [row(planted[0]), row(planted[1]), row(planted[2])]


def run(head_cls, case, pts, gt, loc, rot, pred, dtype):
    """-> (labels (N, S), owner (N, S), loss, tb_dict, gradient) of the reference"""
    head, S = make_head(head_cls, case), case["frames"]
    del base.OWNERS[:]
    tt = lambda a: torch.from_numpy(a).to(dtype)      # noqa: E731
    t = head.assign_targets({"point_coords": tt(pts), "gt_boxes": tt(gt), "locations": tt(loc), "rotations_y": tt(rot)})
    assert len(t) == S and len(base.OWNERS) == 2 * S * B
    owner = np.full((len(pts), S), -1, np.int32)
    for s in range(S):
        for b in range(B):
            owner[pts[:, 0] == b, s] = base.OWNERS[2 * (s * B + b)]
    x = torch.from_numpy(pred.astype(np.float64) / 64).to(dtype).requires_grad_(True)
    head.forward_ret_dict = {"point_cls_preds": x, "point_cls_labels": [d["point_cls_labels"] for d in t]}
    loss, tb = head.get_loss()
    loss.backward()
    return np.stack([d["point_cls_labels"].numpy() for d in t], 1), owner, float(loss.detach()), tb, x.grad.numpy().copy()


def main():
    head_cls, union_boxes = load_reference()
    cuda, flt = torch.Tensor.cuda, torch.Tensor.float
    torch.Tensor.cuda = lambda self, *a, **k: self

    def both(fn):
        """fn(dtype) in float32 and, with .float() as .double(), in float64"""
        a = fn(torch.float32)
        torch.Tensor.float = torch.Tensor.double
        try:
            return a, fn(torch.float64)
        finally:
            torch.Tensor.float = flt
    try:
        for seed in range(700, 760):
            out = {}
            try:
                r = np.random.default_rng(seed + 1000)
                for name, case in mf.CASES.items():
                    S, C = case["frames"], case["num_class"]
                    pts, gt, loc, rot, (moving, ignored, origin) = scene(seed, S, C)
                    mg = mf.margins_mf(pts, gt, loc, rot, mf.EXTRA)
                    mg[origin] = np.inf
                    assert mg.min() >= 1e-4, f"a point within {mg.min():.2e} of a face"
                    pred = np.round(r.normal(0, 3, (len(pts), S * C)) * 64).clip(-1280, 1280)
                    pred[moving], pred[ignored], pred[origin] = 0, 1280, -1280
                    pred[(moving + 1) % len(pts), 0], pred[(ignored + 1) % len(pts), -1] = 1280, 0
                    pred = pred.astype(np.int16)
                    (lab32, own32, l32, tb32, g32), (lab, own, l64, tb64, g64) = both(
                        lambda dt: run(head_cls, case, pts, gt, loc, rot, pred, dt))
                    assert np.array_equal(lab, lab32) and np.array_equal(own, own32)
                    cls2 = int(gt[0, 2, 7])
                    assert lab[moving].tolist() == [1 if C == 1 else cls2, -1, 0][:S] and own[moving].tolist() == [2, -1, -1][:S], "the moving gt"
                    assert (lab[ignored] == -1).all() and (g64[ignored] == 0).all(), "the point ignored in every frame"
                    assert (own[origin] == 4).all() and (lab[origin] == (1 if C == 1 else 0)).all(), "the planted origin point"
                    assert (lab[pts[:, 0] == B] == 0).all() and not (pts[:, 0] == 2).any()
                    assert (lab == -1).sum() > 10 and (lab > 0).sum() > 40
                    if S > 1:
                        mixed = ((lab == -1).any(axis=1) & (lab >= 0).any(axis=1)).sum()
                        assert mixed > 5 and ((lab > 0).any(axis=1) & (lab == 0).any(axis=1)).sum() > 5, "points whose frames disagree"
                    pre = name + "_"
                    out.update({pre + "points": pts, pre + "gt": gt, pre + "loc": loc, pre + "rot": rot, pre + "labels": lab, pre + "owner": own,
                                pre + "pred_cls": pred, pre + "pos": np.int64((lab > 0).sum()), pre + "loss32": np.float64(l32),
                                pre + "loss64": np.float64(l64), pre + "tb32": np.array(json.dumps(tb32)), pre + "tb64": np.array(json.dumps(tb64)),
                                pre + "gcls32": g32, pre + "gcls64": g64, pre + "planted": np.array([moving, ignored, origin], np.int64)})
                    print(f"   {name}: N {len(pts)}, pos {int((lab > 0).sum())}, ignored {int((lab == -1).sum())}, float32 {l32!r}, float64 {l64!r}")
                # the union boxes: a scene with headings beyond +-pi, padding rows, moving and turning gts
                _, gt, loc, rot, _ = scene(seed + 1, 3, 3)
                tt = lambda a, dt: torch.from_numpy(a).to(dt)      # noqa: E731
                e32, e64 = both(lambda dt: union_boxes(tt(gt, dt), tt(loc, dt), tt(rot, dt)).numpy())
                other = both(lambda dt: union_boxes(tt(gt, dt), tt(loc, dt), tt(rot + 0.7, dt)).numpy())
                assert np.array_equal(e32, other[0]) and np.array_equal(e64, other[1]), "rotations_y changed the union boxes"
                assert e64.shape == (B, M, 8) and np.array_equal(e64[..., [0, 1, 2, 5, 6, 7]], gt[..., [0, 1, 2, 5, 6, 7]].astype(np.float64))
                assert (e64[..., 3:5] >= gt[..., 3:5] - 1e-6).all() and (e64[..., 3] > gt[..., 3] + 0.1).any()
                empty = union_boxes(tt(gt[:, :0], torch.float32), tt(loc[:, :0], torch.float32), tt(rot[:, :0], torch.float32))
                assert tuple(empty.shape) == (B, 0, 8)
                out.update(enl_gt=gt, enl_loc=loc, enl_rot=rot, enl32=e32, enl64=e64)
                print(f"   union boxes: max |float32 - float64| {np.abs(e32 - e64).max():.3e}")
                break
            except AssertionError as e:
                print(f"   seed {seed}: {e}")
        else:
            raise RuntimeError("no seed keeps the fixture clear of the thresholds")
    finally:
        torch.Tensor.cuda, torch.Tensor.float = cuda, flt
    out["cases"] = np.array(json.dumps(mf.CASES))
    path = os.path.join(HERE, "point_head_mf_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
