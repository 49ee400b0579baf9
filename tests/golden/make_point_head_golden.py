"""Generates tests/golden/point_head_ref.npz from the REFERENCE ITSELF: its own PointHeadSimple / PointHeadBox /
PointIntraPartOffsetHead (assign_targets -> assign_stack_targets, get_loss) with its own point_head_template, box_coder_utils,
box_utils, common_utils and loss_utils, loaded standalone from their files and run on the CPU.  Runs only where the reference
checkout is (default /root/reference, or $LIDAR_REFERENCE); the .npz is what the tests read.

The heads are built without __init__ (they read model_cfg, num_class, box_coder, box_layers, the loss functions of build_losses and
forward_ret_dict).  Shims, each active only while the reference runs:
  * roiaware_pool3d_utils.points_in_boxes_gpu, the only CUDA call, is oracle.c_oracle.points_in_boxes_gpu: this project's C
    restatement of the CUDA kernel (float32, as the kernel).  The containment test is therefore pinned THROUGH THAT ORACLE
    (tests/test_oracle_pins.py ties it to the reference's kernel); everything the heads do with its answer is the reference's.  The
    stub also records what it returned for the un-enlarged boxes: that is the stored owner index.
  * torch.Tensor.cuda is the identity.
  * current torch's F.binary_cross_entropy refuses targets outside [0, 1]; get_part_layer_loss hands it the part labels of every
    row (a NaN for the planted point a zero-size padding row owns) before it multiplies the non-positive rows by 0.  Such targets
    are passed as 0; the generator asserts that no positive row is concerned, so nothing returned depends on the replacement.
  * the float64 run: rotate_points_along_z ends its matrix in `.float()`, PointResidualCoder stores `.float()` mean sizes and the
    loss methods call `.float()` on their masks; torch.Tensor.float is `.double()` while that run is on, and every input is
    converted to float64 beforehand (exact), so the evaluation is a float64 one.

Each case runs in float32 and in float64, both under autograd.  Stored per case <c>: <c>_points (N, 4), <c>_gt (B, M, 8),
<c>_labels (N) int64, <c>_owner (N) int32, <c>_box{32,64} (N, 8), <c>_part{32,64} (N, 3) where the head has them, <c>_nan (row,
column) of the box label set to NaN before the loss, predictions <c>_pred_{cls,box,part} as int16 on the 1/64 grid,
<c>_loss{32,64} = [cls, box, part] (0 for an absent term), <c>_pos, <c>_tb{32,64} (the tb_dict as JSON) and the gradients
<c>_g{cls,box,part}{32,64} of the SUM the head returns.  `cases`: tests/_point_head_np.py:CASES as JSON.

Scene (B 4, M 10): frame 0 has two overlapping gts first (a planted point in the overlap: the first wins), padding rows, a point
in a shell only, a point in a box, a point far outside, a point exactly at the origin (owned by the first padding row, class 0)
and one 5 cm from it (ignored through the enlarged padding row); frame 1 has no padding; frame 2 only padding rows; frame 3 has
gts and no points (except in the pointrcnn case: the reference's coder with mean sizes takes max() of an empty class tensor and
raises on a frame without a foreground point, so that case gives frame 3 one point inside a gt); one row has bs_idx == B; some headings lie whole turns outside [-pi, pi]; the rows are shuffled.  Logits include
exactly 0 and +-20.

Asserted on the reference's numbers alone, moving to the next seed otherwise: apart from the planted origin point no point lies
within 1e-4 of a face of any box or enlarged box (tests/_point_head_np.py:margins), and no weighted box difference of a positive row
lies within 1e-6 of 1/9.

Usage:  python tests/golden/make_point_head_golden.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _point_head_np as ph  # noqa: E402
from oracle import c_oracle  # noqa: E402

REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refpcdet_ph"
B, M = 4, 10
OWNERS = []


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def to_cfg(d):
    return Cfg({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


def points_in_boxes_stub(points, boxes):
    idx = c_oracle.points_in_boxes_gpu(boxes.detach().numpy(), points.detach().numpy())
    OWNERS.append(idx[0].copy())
    return torch.from_numpy(idx).int()


def load_reference():
    """-> {class name: class} of the reference's three point heads, and its box_coder_utils"""
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
    for sub in ["", ".utils", ".ops", ".ops.roiaware_pool3d", ".ops.iou3d_nms", ".models", ".models.dense_heads"]:
        pkg(PKG + sub, os.path.join(root, *sub.split(".")[1:]))
    sys.modules.setdefault("quaternion", types.ModuleType("quaternion"))
    for stub in [".ops.roiaware_pool3d.roiaware_pool3d_utils", ".ops.iou3d_nms.iou3d_nms_utils"]:
        sys.modules[PKG + stub] = types.ModuleType(PKG + stub)
    sys.modules[PKG + ".ops.roiaware_pool3d.roiaware_pool3d_utils"].points_in_boxes_gpu = points_in_boxes_stub
    sys.modules[PKG + ".ops.roiaware_pool3d"].roiaware_pool3d_utils = sys.modules[PKG + ".ops.roiaware_pool3d.roiaware_pool3d_utils"]
    sys.modules[PKG + ".ops.iou3d_nms"].iou3d_nms_utils = sys.modules[PKG + ".ops.iou3d_nms.iou3d_nms_utils"]
    u = os.path.join(root, "utils")
    load(PKG + ".utils.common_utils", os.path.join(u, "common_utils.py"))
    load(PKG + ".utils.box_utils", os.path.join(u, "box_utils.py"))
    coder = load(PKG + ".utils.box_coder_utils", os.path.join(u, "box_coder_utils.py"))
    load(PKG + ".utils.loss_utils", os.path.join(u, "loss_utils.py"))
    d = os.path.join(root, "models", "dense_heads")
    load(PKG + ".models.dense_heads.point_head_template", os.path.join(d, "point_head_template.py"))
    heads = {}
    for f, c in [("point_head_simple", "PointHeadSimple"), ("point_head_box", "PointHeadBox"), ("point_intra_part_head", "PointIntraPartOffsetHead")]:
        heads[c] = getattr(load(PKG + ".models.dense_heads." + f, os.path.join(d, f + ".py")), c)
    return heads, coder


def make_head(heads, coder, case):
    cls = heads[case["head"]]
    h = cls.__new__(cls)
    nn.Module.__init__(h)
    h.model_cfg, h.num_class = to_cfg(case["cfg"]), case["num_class"]
    t = h.model_cfg.TARGET_CONFIG
    if t.get("BOX_CODER") is not None:
        h.box_coder = getattr(coder, t.BOX_CODER)(**t.BOX_CODER_CONFIG)
    h.box_layers = object() if case["box"] else None
    h.build_losses(h.model_cfg.LOSS_CONFIG)
    return h


def scene(seed, fill_empty_frame):
    """-> points (N, 4), gt (B, M, 8) float32, the row of the planted origin point"""
    r = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    for b, n in ((0, 6), (1, M), (3, 7)):
        gt[b, :n, 0:2] = r.uniform(-18, 18, (n, 2))
        gt[b, :n, 0:2] += np.sign(gt[b, :n, 0:2]) * 3        # nothing real near the origin
        gt[b, :n, 2] = r.uniform(-1.2, 0.2, n)
        k = r.integers(0, 3, n)
        gt[b, :n, 3:6] = np.asarray(ph.MEAN_SIZE, np.float32)[k] * r.uniform(0.85, 1.2, (n, 3))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n) + 2 * np.pi * r.integers(-2, 3, n)
        gt[b, :n, 7] = k + 1
    gt[0, 1] = gt[0, 0]
    gt[0, 1, 0:2] += [0.6, 0.3]                               # overlaps gt 0
    gt[0, 1, 6] += 0.4
    gt[0, 1, 7] = (gt[0, 0, 7] % 3) + 1

    def at(b, k, loc):                                        # a point given in the local frame of gt (b, k), in units of its half dims
        g = gt[b, k].astype(np.float64)
        l3 = np.asarray(loc) * g[3:6] / 2
        c, s = np.cos(g[6]), np.sin(g[6])
        return [b, g[0] + l3[0] * c - l3[1] * s, g[1] + l3[0] * s + l3[1] * c, g[2] + l3[2]]

    g0, g1 = gt[0, 0].astype(np.float64), gt[0, 1].astype(np.float64)
    planted = [[0, *((g0[0:3] + g1[0:3]) / 2)],              # in the overlap of gts 0 and 1: the first wins
               at(0, 2, [1 + 0.1 / gt[0, 2, 3], 0.2, 0.1]),   # 5 cm beyond the x face: shell only
               at(0, 3, [0.3, -0.4, 0.5]),                    # inside a box (and its shell)
               [0, 60.0, 60.0, 5.0],                          # outside everything
               [0, 0.0, 0.0, 0.0],                            # the origin: owned by the first padding row
               [0, 0.05, 0.03, 0.02],                         # ignored through the enlarged padding row
               [2, 0.0, 0.0, 0.0], [2, -0.04, 0.02, 0.05], [2, 5.0, 1.0, 0.0],   # the frame with only padding rows
               [B, 1.0, 1.0, 0.0]]                            # a bs_idx that names no frame
    if fill_empty_frame:
        planted.append(at(3, 0, [0.1, 0.2, -0.3]))
    pts = []
    for b, n in ((0, 420), (1, 520), (2, 60)):
        real = np.nonzero(gt[b, :, 3] > 0)[0]
        bg = np.stack([np.full(n // 3, b), r.uniform(-22, 22, n // 3), r.uniform(-22, 22, n // 3), r.uniform(-2.5, 1.5, n // 3)], 1)
        pts.append(bg)
        if len(real):
            g = gt[b, r.choice(real, n - n // 3)].astype(np.float64)
            xyz = g[:, 0:3] + r.normal(0, 1, (len(g), 3)) * g[:, 3:6] * 0.45
            pts.append(np.concatenate([np.full((len(g), 1), b), xyz], 1))
    pts = np.concatenate(pts + [np.asarray(planted, np.float64)]).astype(np.float32)
    pts = pts[r.permutation(len(pts))]
    origin = np.nonzero((pts[:, 0] == 0) & (pts[:, 1:4] == 0).all(axis=1))[0]
    assert len(origin) == 1
    return pts, gt, int(origin[0])


def run(heads, coder, case, pts, gt, preds, nan_plant, dtype):
    """-> (targets dict of numpy arrays, owner, losses [cls, box, part], tb_dict, gradients dict) of the reference"""
    head = make_head(heads, coder, case)
    del OWNERS[:]
    t = head.assign_targets({"point_coords": torch.from_numpy(pts).to(dtype), "gt_boxes": torch.from_numpy(gt).to(dtype)})
    owner = np.full(len(pts), -1, np.int32)
    for b in range(B):
        owner[pts[:, 0] == b] = OWNERS[2 * b]
    ret = {"point_cls_labels": t["point_cls_labels"]}
    leaves = {}
    for key, lab in (("cls", None), ("box", "point_box_labels"), ("part", "point_part_labels")):
        if preds.get(key) is None:
            continue
        leaves[key] = torch.from_numpy(preds[key].astype(np.float64) / 64).to(dtype).requires_grad_(True)
        ret[f"point_{key}_preds"] = leaves[key]
        if lab:
            ret[lab] = t[lab].clone()
    if nan_plant is not None:
        ret["point_box_labels"][nan_plant[0], nan_plant[1]] = float("nan")
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    loss.backward()
    losses = np.array([tb["point_loss_cls"], tb.get("point_loss_box", 0.0), tb.get("point_loss_part", 0.0)], np.float64)
    tn = {k: (None if v is None else v.numpy().copy()) for k, v in t.items()}
    return tn, owner, losses, tb, {k: v.grad.numpy().copy() for k, v in leaves.items()}


def predictions(r, case, t64, nan_row):
    """int16 grid values (x 1/64): logits N(0, 3) with planted 0 and +-20, box predictions around the labels, part logits N(0, 2)"""
    n = len(t64["point_cls_labels"])
    cls = np.round(r.normal(0, 3, (n, case["num_class"])) * 64).clip(-1280, 1280)
    pos = np.nonzero(t64["point_cls_labels"] > 0)[0]
    neg = np.nonzero(t64["point_cls_labels"] == 0)[0]
    for rows in (pos, neg):
        cls[rows[0]], cls[rows[1]], cls[rows[2]] = 0, 1280, -1280
    out = dict(cls=cls.astype(np.int16), box=None, part=None)
    if case["box"]:
        lab = np.nan_to_num(t64["point_box_labels"], nan=0.0, posinf=0.0, neginf=0.0)
        out["box"] = np.round((lab + r.normal(0, 0.12, (n, 8))) * 64).clip(-2000, 2000).astype(np.int16)
        out["box"][pos[3]] = np.round(lab[pos[3]] * 64)        # differences below 1/128: the quadratic branch, some exactly 0
    if case["part"]:
        out["part"] = np.round(r.normal(0, 2, (n, 3)) * 64).astype(np.int16)
        out["part"][pos[0]] = 0
    return out


def main():
    heads, coder = load_reference()
    cuda, flt, bce = torch.Tensor.cuda, torch.Tensor.float, torch.nn.functional.binary_cross_entropy
    torch.Tensor.cuda = lambda self, *a, **k: self
    replaced = []

    def bce_shim(x, t, *a, **k):
        bad = ~((t >= 0) & (t <= 1))
        replaced.append(bad.any(dim=-1))
        return bce(x, torch.where(bad, torch.zeros_like(t), t), *a, **k)
    torch.nn.functional.binary_cross_entropy = bce_shim
    try:
        for seed in range(500, 540):
            out = {}
            try:
                r = np.random.default_rng(seed + 1000)
                for name, case in ph.CASES.items():
                    pts, gt, origin = scene(seed, fill_empty_frame=name == "pointrcnn")
                    extra = case["cfg"]["TARGET_CONFIG"]["GT_EXTRA_WIDTH"]
                    mg = ph.margins(pts, gt, extra)
                    mg[origin] = np.inf
                    mg[(pts[:, 0] == 2) & (pts[:, 1:4] == 0).all(axis=1)] = np.inf      # the origin point of the padding-only frame
                    assert mg.min() >= 1e-4, f"a point within {mg.min():.2e} of a face"
                    # targets first (float64, no predictions needed), then predictions around them
                    torch.Tensor.float = torch.Tensor.double
                    try:
                        head = make_head(heads, coder, case)
                        del OWNERS[:]
                        t0 = head.assign_targets({"point_coords": torch.from_numpy(pts).double(), "gt_boxes": torch.from_numpy(gt).double()})
                        t0 = {k: (None if v is None else v.numpy()) for k, v in t0.items()}
                    finally:
                        torch.Tensor.float = flt
                    pos = np.nonzero(t0["point_cls_labels"] > 0)[0]
                    preds = predictions(r, case, t0, None)
                    nan_plant = (int(pos[5]), 4) if case["box"] else None
                    if case["box"]:
                        cw = np.asarray(case["cfg"]["LOSS_CONFIG"]["LOSS_WEIGHTS"]["code_weights"])
                        d = np.abs((preds["box"][pos] / 64 - t0["point_box_labels"][pos]) * cw)
                        assert (np.abs(d[np.isfinite(d)] - 1 / 9) >= 1e-6).all(), "a weighted box difference within 1e-6 of 1/9"
                    del replaced[:]
                    t32, own32, l32, tb32, g32 = run(heads, coder, case, pts, gt, preds, nan_plant, torch.float32)
                    torch.Tensor.float = torch.Tensor.double
                    try:
                        t64, own64, l64, tb64, g64 = run(heads, coder, case, pts, gt, preds, nan_plant, torch.float64)
                    finally:
                        torch.Tensor.float = flt
                    lab = t64["point_cls_labels"]
                    assert np.array_equal(lab, t32["point_cls_labels"]) and np.array_equal(own32, own64)
                    for bad in replaced:
                        assert not bad.numpy()[lab > 0].any(), "a positive row with a part label outside [0, 1]"
                    assert lab[origin] == (1 if case["num_class"] == 1 else 0) and own64[origin] == 6, "the planted origin point"
                    assert (lab == -1).sum() > 20 and (lab > 0).sum() > 50
                    out[f"{name}_points"], out[f"{name}_gt"] = pts, gt
                    out[f"{name}_labels"], out[f"{name}_owner"], out[f"{name}_pos"] = lab, own64, np.int64((lab > 0).sum())
                    for tag, t, l, tb, g in (("32", t32, l32, tb32, g32), ("64", t64, l64, tb64, g64)):
                        if case["box"]:
                            out[f"{name}_box{tag}"] = t["point_box_labels"]
                        if case["part"]:
                            out[f"{name}_part{tag}"] = t["point_part_labels"]
                        out[f"{name}_loss{tag}"], out[f"{name}_tb{tag}"] = l, np.array(json.dumps(tb))
                        for k, v in g.items():
                            out[f"{name}_g{k}{tag}"] = v
                    for k, v in preds.items():
                        if v is not None:
                            out[f"{name}_pred_{k}"] = v
                    if nan_plant:
                        out[f"{name}_nan"] = np.array(nan_plant, np.int64)
                    print(f"   {name}: N {len(pts)}, pos {int((lab > 0).sum())}, ignored {int((lab == -1).sum())}, owned by a padding row "
                          f"{int(((own64 >= 0) & (gt[np.clip(pts[:, 0].astype(int), 0, B - 1), np.maximum(own64, 0), 3] == 0)).sum())}\n"
                          f"      float32 {l32.tolist()}\n      float64 {l64.tolist()}")
                break
            except AssertionError as e:
                print(f"   seed {seed}: {e}")
        else:
            raise RuntimeError("no seed keeps the fixture clear of the thresholds")
    finally:
        torch.Tensor.cuda, torch.Tensor.float, torch.nn.functional.binary_cross_entropy = cuda, flt, bce
    out["cases"] = np.array(json.dumps(ph.CASES))
    path = os.path.join(HERE, "point_head_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
