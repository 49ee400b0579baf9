"""Generates tests/golden/anchor_assign_ref.npz from the REFERENCE ITSELF: its own AxisAlignedTargetAssigner
(pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py), AnchorGenerator (anchor_generator.py) and
ResidualCoder (pcdet/utils/box_coder_utils.py), loaded standalone from their files and run on the CPU.  Runs only where the
reference checkout is (default /root/reference, or $LIDAR_REFERENCE); the .npz (inputs, anchors, outputs) is what the GPU tests read.

The modules the path under test never calls are stubs: `quaternion` (imported by common_utils), and the CUDA extension
wrappers iou3d_nms_utils / roiaware_pool3d_utils (MATCH_HEIGHT is False, so boxes_iou3d_gpu is not reached).
torch.Tensor.cuda is the identity while the reference runs.

Cases
  kitti    PointPillar-KITTI anchors (pointpillar.yaml) on a 48 x 40 map, bs 4, single head: a frame of only padding, a trailing
           row that sums to 0 without being zero, a class absent from a frame, gts exactly on anchors (ties at the gt max), two
           identical gts, a gt outside the anchor range, headings 1 ulp either side of +-pi/4 and +-3pi/4, a class-0 gt
  kitti_norm   the same with NORM_BY_NUM_EXAMPLES True and gt_boxes_enlarged (dims + 0.2) passed
  kitti_inverted   the same gts with Car's matched threshold below its unmatched one (targets of label-0 anchors)
  nus      NuScenes-style USE_MULTIHEAD, 10 classes, ResidualCoder(code_size=9, encode_angle_by_sincos=True), 9-column gts with
           velocity, anchors zero-padded to code_size columns, bs 2 (SEPARATE_MULTIHEAD spelled as the configs do: not read)
  nus_remap    the same with the key the reference reads, SEPERATE_MULTIHEAD True, and RPN_HEAD_CFGS

Usage:  python tests/golden/make_assign_golden.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refpcdet_assign"


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def load_reference():
    """-> (axis_aligned_target_assigner, anchor_generator, box_coder_utils) modules of the reference"""
    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
        return m

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
    for stub in [".ops.iou3d_nms.iou3d_nms_utils", ".ops.roiaware_pool3d.roiaware_pool3d_utils"]:
        sys.modules[PKG + stub] = types.ModuleType(PKG + stub)
    load(PKG + ".utils.common_utils", os.path.join(root, "utils", "common_utils.py"))
    load(PKG + ".utils.box_utils", os.path.join(root, "utils", "box_utils.py"))
    coder = load(PKG + ".utils.box_coder_utils", os.path.join(root, "utils", "box_coder_utils.py"))
    ta = os.path.join(root, "models", "dense_heads", "target_assigner")
    gen = load(PKG + ".models.dense_heads.target_assigner.anchor_generator", os.path.join(ta, "anchor_generator.py"))
    asg = load(PKG + ".models.dense_heads.target_assigner.axis_aligned_target_assigner",
               os.path.join(ta, "axis_aligned_target_assigner.py"))
    return asg, gen, coder


KITTI_RANGE = [0, -39.68, -3, 69.12, 39.68, 1]
KITTI_CFG = [  # pointpillar.yaml ANCHOR_GENERATOR_CONFIG
    dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
         align_center=False, feature_map_stride=2, matched_threshold=0.6, unmatched_threshold=0.45),
    dict(class_name="Pedestrian", anchor_sizes=[[0.8, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
         align_center=False, feature_map_stride=2, matched_threshold=0.5, unmatched_threshold=0.35),
    dict(class_name="Cyclist", anchor_sizes=[[1.76, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
         align_center=False, feature_map_stride=2, matched_threshold=0.5, unmatched_threshold=0.35),
]
KITTI_NAMES = ["Car", "Pedestrian", "Cyclist"]

NUS_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
NUS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
             "traffic_cone"]
NUS_SIZES = [[4.63, 1.97, 1.74], [6.93, 2.51, 2.84], [6.37, 2.85, 3.19], [10.5, 2.94, 3.47], [12.29, 2.90, 3.87],
             [0.50, 2.53, 0.98], [2.11, 0.77, 1.47], [1.70, 0.60, 1.28], [0.73, 0.67, 1.77], [0.41, 0.41, 1.07]]
NUS_BOTTOM = [-0.95, -0.6, -0.225, -0.085, 0.115, -1.33, -1.085, -1.18, -0.935, -1.285]
NUS_THRESH = [(0.6, 0.45), (0.55, 0.4), (0.5, 0.35), (0.55, 0.4), (0.5, 0.35), (0.55, 0.4), (0.5, 0.3), (0.5, 0.35),
              (0.6, 0.4), (0.6, 0.4)]
NUS_CFG = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[h], align_center=False,
                feature_map_stride=4, matched_threshold=t[0], unmatched_threshold=t[1])
           for n, s, h, t in zip(NUS_NAMES, NUS_SIZES, NUS_BOTTOM, NUS_THRESH)]
NUS_HEADS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"],
             ["pedestrian", "traffic_cone"]]


def f32_next(x, direction):
    return float(np.nextafter(np.float32(x), np.float32(direction)))


def kitti_gt(anchors):
    """(4, 12, 8) gt boxes with classes, the edge cases of the module docstring"""
    r = np.random.default_rng(11)
    B, M = 4, 12
    gt = np.zeros((B, M, 8), np.float32)
    flat = [a.reshape(-1, 7).numpy() for a in anchors]

    def rand_box(cls):
        size = np.array(KITTI_CFG[cls - 1]["anchor_sizes"][0]) * r.uniform(0.8, 1.2, 3)
        return [r.uniform(2, 67), r.uniform(-37, 37), r.uniform(-2, 0), *size, r.uniform(-np.pi, np.pi), cls]

    # frame 0: gts exactly on anchors (ties), two identical gts, a gt outside the range, headings around +-pi/4, +-3pi/4, and a
    # trailing row [1, -1, 0, ...] that sums to 0 (trimmed with the padding behind it)
    q = np.pi / 4
    rows = [[*flat[0][1000], 1], [*flat[1][2222], 2], [*flat[2][3001], 3], [*flat[0][1000], 1],
            [200.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 1],
            [20.0, 5.0, -1.0, 3.9, 1.6, 1.56, f32_next(q, 0), 1], [24.0, -5.0, -1.0, 3.9, 1.6, 1.56, f32_next(q, 10), 1],
            [30.0, 10.0, -0.6, 1.76, 0.6, 1.73, f32_next(-3 * q, 0), 3], [34.0, -10.0, -0.6, 1.76, 0.6, 1.73, f32_next(-3 * q, -10), 3],
            [40.0, 12.0, -0.6, 0.8, 0.6, 1.73, f32_next(3 * q, 0), 2], [1.0, -1.0, 0, 0, 0, 0, 0, 2]]
    gt[0, :len(rows)] = np.array(rows, np.float32)
    # frame 1: only padding
    # frame 2: no Pedestrian, 5 gts
    gt[2, :5] = np.array([rand_box(c) for c in [1, 3, 1, 3, 1]], np.float32)
    # frame 3: 10 gts, one of them with class id 0 (wraps to the last class name, label 0), another one exactly on an anchor
    gt[3, :10] = np.array([rand_box(c) for c in [1, 2, 3, 1, 2, 3, 1, 1, 2, 3]], np.float32)
    gt[3, 4, 7] = 0
    gt[3, 6] = np.array([*flat[0][3431], 1], np.float32)
    return gt


def nus_gt(anchors):
    r = np.random.default_rng(12)
    B, M = 2, 30
    gt = np.zeros((B, M, 10), np.float32)
    for b, n in enumerate([30, 17]):
        for j in range(n):
            c = int(r.integers(1, 11))
            size = np.array(NUS_SIZES[c - 1]) * r.uniform(0.8, 1.2, 3)
            gt[b, j] = [r.uniform(-48, 48), r.uniform(-48, 48), r.uniform(-2, 1), *size, r.uniform(-np.pi, np.pi),
                        *r.normal(0, 3, 2), c]
    # one gt exactly on an anchor of class 4 (bus); its velocity columns stay
    a = anchors[3].permute(3, 4, 0, 1, 2, 5).reshape(-1, anchors[3].shape[-1]).numpy()
    gt[0, 5, :7] = a[77, :7]
    gt[0, 5, 9] = 4
    return gt


def build_case(gen, coder, cfg, pc_range, grid, multihead=False, seperate=False, norm=False, code_size=7, sincos=False):
    """-> (the reference's anchors for `cfg`, padded to code_size columns as its anchor head does; its ResidualCoder; a model
    config for its AxisAlignedTargetAssigner).  Nothing is assigned here."""
    box_coder = coder.ResidualCoder(code_size=code_size, encode_angle_by_sincos=sincos)
    ag = gen.AnchorGenerator(anchor_range=pc_range, anchor_generator_config=cfg)
    anchors, _ = ag.generate_anchors([grid] * len(cfg))
    if box_coder.code_size != 7:   # anchor_head_template.generate_anchors: zero columns up to anchor_ndim = code_size
        anchors = [torch.cat((a, a.new_zeros([*a.shape[:-1], box_coder.code_size - 7])), dim=-1) for a in anchors]
    model_cfg = Cfg(ANCHOR_GENERATOR_CONFIG=cfg, USE_MULTIHEAD=multihead,
                    TARGET_ASSIGNER_CONFIG=Cfg(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                               NORM_BY_NUM_EXAMPLES=norm, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"))
    if multihead:
        model_cfg["SEPARATE_MULTIHEAD" if not seperate else "SEPERATE_MULTIHEAD"] = True
        model_cfg["RPN_HEAD_CFGS"] = [dict(HEAD_CLS_NAME=h) for h in NUS_HEADS]
    return anchors, box_coder, model_cfg


def main():
    asg, gen, coder = load_reference()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        cases = []
        # KITTI single head
        anchors, _, _ = build_case(gen, coder, KITTI_CFG, KITTI_RANGE, [48, 40])
        kgt = kitti_gt(anchors)
        kenl = kgt.copy()
        kenl[:, :, 3:6] += 0.2
        cases.append(("kitti", dict(names=KITTI_NAMES, cfg=KITTI_CFG, pc_range=KITTI_RANGE, grid=[48, 40], gt=kgt)))
        cases.append(("kitti_norm", dict(names=KITTI_NAMES, cfg=KITTI_CFG, pc_range=KITTI_RANGE, grid=[48, 40], gt=kgt, norm=True,
                                         enlarged=kenl)))
        # matched < unmatched for Car: the reference encodes targets for anchors its later background pass labels 0
        inverted = [dict(KITTI_CFG[0], matched_threshold=0.3, unmatched_threshold=0.55)] + KITTI_CFG[1:]
        cases.append(("kitti_inverted", dict(names=KITTI_NAMES, cfg=inverted, pc_range=KITTI_RANGE, grid=[48, 40], gt=kgt)))
        anchors, _, _ = build_case(gen, coder, NUS_CFG, NUS_RANGE, [16, 16], code_size=9, sincos=True)
        ngt = nus_gt(anchors)
        for name, sep in [("nus", False), ("nus_remap", True)]:
            cases.append((name, dict(names=NUS_NAMES, cfg=NUS_CFG, pc_range=NUS_RANGE, grid=[16, 16], gt=ngt, multihead=True,
                                     seperate=sep, code_size=9, sincos=True)))
        for name, c in cases:
            kw = {k: c[k] for k in ["multihead", "seperate", "norm", "code_size", "sincos"] if k in c}
            anchors, box_coder, model_cfg = build_case(gen, coder, c["cfg"], c["pc_range"], c["grid"], **kw)
            a = asg.AxisAlignedTargetAssigner(model_cfg, class_names=c["names"], box_coder=box_coder, match_height=False)
            enl = torch.from_numpy(c["enlarged"]) if c.get("enlarged") is not None else None
            res = a.assign_targets(anchors, torch.from_numpy(c["gt"]), gt_boxes_enlarged=enl)
            meta = dict(class_names=c["names"], anchor_generator_config=c["cfg"], pc_range=c["pc_range"], grid=c["grid"],
                        use_multihead=bool(c.get("multihead", False)), seperate_multihead=bool(c.get("seperate", False)),
                        rpn_head_cfgs=[dict(HEAD_CLS_NAME=h) for h in NUS_HEADS] if c.get("multihead") else None,
                        norm_by_num_examples=bool(c.get("norm", False)), code_size=c.get("code_size", 7),
                        encode_angle_by_sincos=bool(c.get("sincos", False)), num_anchors=len(anchors))
            out[f"{name}_meta"] = np.array(json.dumps(meta))
            out[f"{name}_gt"] = c["gt"]
            if enl is not None:
                out[f"{name}_gt_enlarged"] = c["enlarged"]
            for k, t in enumerate(anchors):
                out[f"{name}_anchors_{k}"] = t.numpy()
            out[f"{name}_labels"] = res["box_cls_labels"].numpy()
            out[f"{name}_targets"] = res["box_reg_targets"].numpy()
            out[f"{name}_weights"] = res["reg_weights"].numpy()
            lab = res["box_cls_labels"]
            print(name, tuple(lab.shape), "pos", int((lab > 0).sum()), "neg", int((lab == 0).sum()), "ignored", int((lab < 0).sum()))
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "anchor_assign_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
