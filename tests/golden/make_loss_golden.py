"""Generates tests/golden/anchor_loss_ref.npz from the REFERENCE ITSELF: its own AnchorHeadTemplate.get_loss / AnchorHeadMulti.get_loss
(pcdet/models/dense_heads/anchor_head_template.py, anchor_head_multi.py) with its own loss_utils.py, on labels and targets from its
own AxisAlignedTargetAssigner, loaded standalone from their files and run on the CPU.  Runs only where a reference checkout is (found
as make_assign_golden.py finds it); the .npz is what the tests read.

The heads are built without __init__ (no convolutions, no anchor generation on the device): the loss methods read model_cfg,
num_class, anchors, num_anchors_per_location, use_multihead, separate_multihead, rpn_heads[i].num_class and forward_ret_dict, and
build_losses() makes the loss modules.  Modules the loss never calls are stubs (BaseBEVBackbone, ATSSTargetAssigner, the CUDA
extension wrappers); torch.Tensor.cuda is the identity while the reference runs.

Each case runs get_loss twice: in fp32 (the losses), and with the predictions in fp64 under autograd (the losses and the gradients
with respect to every prediction, stored in fp32 with a bit mask of their exact zeros; labels, targets and anchors stay fp32,
so the direction targets are the fp32 ones).  Predictions
lie on a 1/64 grid (exact in fp32), with planted values: logits exactly 0 and beyond +-30, a box difference exactly fp32(1/9) and
one exactly 0, headings at the direction-bin edges; a frame without positives, label -1 anchors and (multi) a positive labelled
with another head's class.

Cases
  kitti        AnchorHeadSingle-style template, pointpillar.yaml: 3 classes, code 7, dir classifier, 12 x 10 map, bs 3
  agnostic     the same anchors and labels with num_class 1 (positives relabelled to 1 in place)
  nodir        the template without a direction classifier (add_sin_difference still applied)
  kitti_multi  kitti second_multihead.yaml-style AnchorHeadMulti: SEPARATE_MULTIHEAD, a head per class, dir classifier
  nus          cbgs_second_multihead.yaml-style: 10 classes in 6 heads, sincos code 10, WeightedL1Loss, pos/neg class weight 1/2,
               velocity code weights 0.2, NaN velocity targets, no direction classifier, 8 x 8 map, bs 2
  multi_nosep  AnchorHeadMulti without SEPARATE_MULTIHEAD: one concatenated prediction over all num_class columns

Usage:  python tests/golden/make_loss_golden.py
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
sys.path.insert(0, HERE)
import make_assign_golden as mag  # noqa: E402

REF = mag.REF
PKG = mag.PKG
Cfg = mag.Cfg

PP_LOSS = dict(LOSS_WEIGHTS={"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2, "code_weights": [1.0] * 7})
NUS_LOSS = dict(REG_LOSS_TYPE="WeightedL1Loss",
                LOSS_WEIGHTS={"pos_cls_weight": 1.0, "neg_cls_weight": 2.0, "cls_weight": 1.0, "loc_weight": 0.25,
                              "dir_weight": 0.2, "code_weights": [1.0] * 8 + [0.2, 0.2]})
KITTI_HEADS = [["Car"], ["Pedestrian"], ["Cyclist"]]
DIR_OFFSET = 0.78539


def load_reference():
    """-> (assigner, generator, coder, anchor_head_template, anchor_head_multi) modules of the reference"""
    asg, gen, coder = mag.load_reference()
    root = os.path.join(REF, "pcdet")

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    bb = types.ModuleType(PKG + ".models.backbones_2d")
    bb.BaseBEVBackbone = nn.Module
    sys.modules[PKG + ".models.backbones_2d"] = bb
    atss = types.ModuleType(PKG + ".models.dense_heads.target_assigner.atss_target_assigner")
    atss.ATSSTargetAssigner = None
    sys.modules[atss.__name__] = atss
    load(PKG + ".utils.loss_utils", os.path.join(root, "utils", "loss_utils.py"))
    dh = os.path.join(root, "models", "dense_heads")
    tmpl = load(PKG + ".models.dense_heads.anchor_head_template", os.path.join(dh, "anchor_head_template.py"))
    multi = load(PKG + ".models.dense_heads.anchor_head_multi", os.path.join(dh, "anchor_head_multi.py"))
    return asg, gen, coder, tmpl, multi


def on_grid(r, shape, scale):
    return (np.round(r.normal(0, scale, shape) * 64) / 64).astype(np.float32)


def gts_on_anchors(r, flat, per_class, cls_ids, B, M, gt_cols, empty_frame, nan_velocity=False):
    """gts near anchors of their class (so they match), a few random ones; frame `empty_frame` holds only padding"""
    gt = np.zeros((B, M, gt_cols), np.float32)
    for b in range(B):
        if b == empty_frame:
            continue
        n = int(r.integers(M // 2, M + 1))
        for j in range(n):
            c = int(r.choice(cls_ids))
            a = flat[c - 1][int(r.integers(0, len(flat[c - 1])))]
            box = a[:7].copy()
            box[:2] += r.uniform(-0.3, 0.3, 2)
            box[3:6] *= r.uniform(0.9, 1.1, 3)
            box[6] = r.uniform(-np.pi, np.pi)
            gt[b, j, :7] = box
            if gt_cols > 8:
                gt[b, j, 7:gt_cols - 1] = r.normal(0, 3, gt_cols - 8)
                if nan_velocity and j % 3 == 0:
                    gt[b, j, 7:gt_cols - 1] = np.nan
            gt[b, j, -1] = c
    return gt


def make_head(tmpl, multi, kind, model_cfg, num_class, anchors, per_loc, head_nc=None):
    cls = multi.AnchorHeadMulti if kind == "multi" else tmpl.AnchorHeadTemplate
    h = cls.__new__(cls)
    nn.Module.__init__(h)
    h.model_cfg = model_cfg
    h.num_class = num_class
    h.use_multihead = model_cfg.get("USE_MULTIHEAD", False)
    h.anchors = anchors
    h.num_anchors_per_location = sum(per_loc)       # AnchorHeadSingle sums the per-class counts
    h.forward_ret_dict = {}
    if kind == "multi":
        h.separate_multihead = model_cfg.get("SEPARATE_MULTIHEAD", False)
        h.rpn_heads = [types.SimpleNamespace(num_class=c) for c in head_nc]
    h.build_losses(model_cfg.LOSS_CONFIG)
    return h


def run_loss(head, preds, labels, targets, dtype):
    """-> (cls, loc, dir, rpn) losses as floats, tb_dict, labels after the call, predictions (for their .grad)"""
    ps = {k: ([t.to(dtype).requires_grad_(dtype == torch.float64) for t in v] if isinstance(v, list) else
              v.to(dtype).requires_grad_(dtype == torch.float64)) for k, v in preds.items() if v is not None}
    head.forward_ret_dict = dict(ps, box_cls_labels=labels.clone(), box_reg_targets=targets.clone())
    loss, tb = head.get_loss()
    if dtype == torch.float64:
        loss.backward()
    return loss, tb, head.forward_ret_dict["box_cls_labels"], ps


def main():
    asg, gen, coder, tmpl, multi = load_reference()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        for name in ["kitti", "agnostic", "nodir", "kitti_multi", "nus", "multi_nosep"]:
            r = np.random.default_rng(sum(map(ord, name)))
            nus = name == "nus"
            multihead = name in ("kitti_multi", "nus", "multi_nosep")
            if nus:
                cfg, names, pc_range, grid, B, M = mag.NUS_CFG, mag.NUS_NAMES, mag.NUS_RANGE, [8, 8], 2, 16
                code_size, sincos, heads = 9, True, mag.NUS_HEADS
            else:
                cfg, names, pc_range, grid, B, M = mag.KITTI_CFG, mag.KITTI_NAMES, mag.KITTI_RANGE, [12, 10], 3, 8
                code_size, sincos, heads = 7, False, KITTI_HEADS
            if name == "agnostic":
                cfg, names = cfg[:1], names[:1]
            anchors, box_coder, acfg = mag.build_case(gen, coder, cfg, pc_range, grid, multihead=multihead, code_size=code_size,
                                                      sincos=sincos)
            if multihead:   # the assigner reads SEPERATE_MULTIHEAD (not set here): labels are the gts' own class ids
                acfg["RPN_HEAD_CFGS"] = [dict(HEAD_CLS_NAME=h) for h in heads]
                acfg.pop("SEPARATE_MULTIHEAD", None)
            a = asg.AxisAlignedTargetAssigner(acfg, class_names=names, box_coder=box_coder, match_height=False)
            flat = [(x.permute(3, 4, 0, 1, 2, 5) if multihead else x).reshape(-1, x.shape[-1]).numpy() for x in anchors]
            gt = gts_on_anchors(r, flat, None, list(range(1, len(names) + 1)), B, M, 10 if nus else 8, empty_frame=1,
                                nan_velocity=nus)
            res = a.assign_targets(anchors, torch.from_numpy(gt))
            labels, targets = res["box_cls_labels"].clone(), res["box_reg_targets"].clone()
            # the anchors in the loss's order (get_box_reg_layer_loss :175-184)
            if multihead:
                cat = torch.cat([x.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, x.shape[-1]) for x in anchors], dim=0)
            else:
                cat = torch.cat(anchors, dim=-3)
            cat = cat.reshape(-1, cat.shape[-1])
            N = cat.shape[0]
            per_loc = [len(c["anchor_sizes"]) * len(c["anchor_rotations"]) * len(c["anchor_bottom_heights"]) for c in cfg]
            use_dir = name not in ("nodir", "nus")
            loss_cfg = Cfg(NUS_LOSS if nus else PP_LOSS)
            loss_cfg["LOSS_WEIGHTS"] = dict(loss_cfg["LOSS_WEIGHTS"])
            model_cfg = Cfg(LOSS_CONFIG=loss_cfg, DIR_OFFSET=DIR_OFFSET, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                            USE_MULTIHEAD=multihead)
            if use_dir:
                model_cfg["USE_DIRECTION_CLASSIFIER"] = True
            if name in ("kitti_multi", "nus"):
                model_cfg["SEPARATE_MULTIHEAD"] = True
            num_class = len(names)
            # positives and the planted edge cases
            pos = torch.nonzero(labels > 0)
            if len(pos) < 8:
                raise RuntimeError(f"{name}: only {len(pos)} positives")
            (b0, i0), (b1, i1), (b2, i2) = pos[0].tolist(), pos[len(pos) // 2].tolist(), pos[-1].tolist()
            labels[0, 5] = -1                               # ignored anchors besides the assigner's own
            labels[2 if B > 2 else 0, N - 3] = -1
            if name in ("kitti_multi", "nus"):              # a positive labelled with another head's class
                n0 = flat[0].shape[0]
                labels[0, n0 + 2] = 1
            # predictions in the reference's views
            code = targets.shape[-1]
            if multihead:
                sizes = []
                k = 0
                for h in heads:
                    n = sum(flat[names.index(c)].shape[0] for c in h)
                    sizes.append(n)
                    k += n
                assert k == N
                sep = name != "multi_nosep"
                head_nc = [len(h) if sep else num_class for h in heads]
                if sep:
                    cls_p = [torch.from_numpy(on_grid(r, (B, n, c), 3.0)) for n, c in zip(sizes, head_nc)]
                    box_p = [torch.from_numpy(on_grid(r, (B, n, code), 0.6)) for n in sizes]
                    dir_p = [torch.from_numpy(on_grid(r, (B, n, 2), 2.0)) for n in sizes] if use_dir else None
                else:
                    cls_p = torch.from_numpy(on_grid(r, (B, N, num_class), 3.0))
                    box_p = torch.from_numpy(on_grid(r, (B, N, code), 0.6))
                    dir_p = torch.from_numpy(on_grid(r, (B, N, 2), 2.0)) if use_dir else None
            else:
                head_nc = None
                H, W = anchors[0].shape[1], anchors[0].shape[2]
                A = sum(per_loc)
                cls_p = torch.from_numpy(on_grid(r, (B, H, W, A * num_class), 3.0))
                box_p = torch.from_numpy(on_grid(r, (B, H, W, A * code), 0.6))
                dir_p = torch.from_numpy(on_grid(r, (B, H, W, A * 2), 2.0)) if use_dir else None
            first = lambda x: x[0] if isinstance(x, list) else x    # noqa: E731
            c0 = first(cls_p).view(B, -1)
            c0[b0, :4] = torch.tensor([0.0, -0.0, 30.0, -30.0])     # logits exactly 0 and |x| >= 30
            c0[b1, 7:10] = torch.tensor([31.5, -40.0, 0.0])
            bx = first(box_p).reshape(B, -1, code)
            if b0 < bx.shape[0] and i0 < bx.shape[1]:
                targets[b0, i0, 2] = 0.0
                bx[b0, i0, 2] = float(np.float32(1.0 / 9.0))         # |diff| exactly fp32(1/9), code weight 1
                bx[b0, i0, 1] = float(targets[b0, i0, 1])            # diff exactly 0
            if use_dir:                                              # headings at the bin edges: t6 + a6 - DIR_OFFSET = 0, pi
                off = np.float32(DIR_OFFSET)
                for (bb, ii), t6 in zip(pos[1:7].tolist(), [off, np.nextafter(off, np.float32(0)), np.nextafter(off, np.float32(9)),
                                                            np.float32(np.pi) + off, np.nextafter(np.float32(np.pi) + off, np.float32(0)),
                                                            np.float32(-np.pi) + off]):
                    targets[bb, ii, 6] = float(np.float32(t6) - np.float32(cat[ii, 6]))
            preds = dict(cls_preds=cls_p, box_preds=box_p, dir_cls_preds=dir_p)
            head = make_head(tmpl, multi, "multi" if multihead else "template", model_cfg, num_class, anchors, per_loc, head_nc)
            l32, tb32, lab_after, _ = run_loss(head, preds, labels, targets, torch.float32)
            l64, tb64, _, p64 = run_loss(head, preds, labels, targets, torch.float64)
            meta = dict(kind="multi" if multihead else "template", num_class=num_class, class_names=list(names),
                        head_num_classes=head_nc, heads=[list(h) for h in heads] if multihead else None,
                        separate=name in ("kitti_multi", "nus"), use_dir=use_dir, model_cfg=model_cfg,
                        anchor_generator_config=cfg, pc_range=pc_range, grid=grid, batch=B, code_size=code,
                        listed=isinstance(cls_p, list), tb32=tb32, tb64=tb64)
            out[f"{name}_meta"] = np.array(json.dumps(meta))
            out[f"{name}_labels"] = labels.numpy()
            out[f"{name}_labels_after"] = lab_after.numpy()
            out[f"{name}_targets"] = targets.numpy()
            out[f"{name}_anchors"] = cat.numpy()
            out[f"{name}_gt"] = gt
            out[f"{name}_loss32"] = np.array([tb32["rpn_loss_cls"], tb32["rpn_loss_loc"], tb32.get("rpn_loss_dir", 0.0)])
            out[f"{name}_loss64"] = np.array([tb64["rpn_loss_cls"], tb64["rpn_loss_loc"], tb64.get("rpn_loss_dir", 0.0)])
            for key, short in [("cls_preds", "cls"), ("box_preds", "box"), ("dir_cls_preds", "dir")]:
                v = preds[key]
                if v is None:
                    continue
                vs, gs = (v, p64[key]) if isinstance(v, list) else ([v], [p64[key]])
                for k, (x, gx) in enumerate(zip(vs, gs)):
                    out[f"{name}_{short}_{k}"] = x.numpy()
                    out[f"{name}_g{short}_{k}"] = gx.grad.numpy().astype(np.float32)
                    out[f"{name}_z{short}_{k}"] = np.packbits(gx.grad.numpy() == 0)   # exact zeros (fp32 storage flushes tiny ones)
            print(name, "N", N, "pos", int((labels > 0).sum()), "ignored", int((labels < 0).sum()), "losses32",
                  out[f"{name}_loss32"], "losses64", out[f"{name}_loss64"])
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "anchor_loss_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
