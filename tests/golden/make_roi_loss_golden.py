"""Generates tests/golden/roi_loss_ref.npz from the REFERENCE ITSELF: its own RoIHeadTemplate.get_loss
(pcdet/models/roi_heads/roi_head_template.py:133-233) with its own loss_utils, box_coder_utils, box_utils and common_utils, loaded
standalone from their files and run on the CPU.  Runs only where the reference checkout is (default /root/reference, or
$LIDAR_REFERENCE); the .npz is what the tests read.

The head is built without __init__ (it reads model_cfg, box_coder, reg_loss_func and forward_ret_dict); modules the loss never calls
are empty stubs (quaternion, the CUDA extension wrappers, model_nms_utils, the ProposalTargetLayer); torch.Tensor.cuda is the identity while the
reference runs.  The targets are the reference's own ProposalTargetLayer + assign_targets outputs stored in
proposal_target_ref.npz, cut to frames and planted as tests/_roi_loss_torch.py:case_targets says (the file does not repeat them).

Each case runs three ways: float32; float32 under autograd; everything in float64 under autograd.  One shim for the last:
rotate_points_along_z ends its rotation matrix in `.float()`, which torch refuses to multiply with float64 points, so
torch.Tensor.float is `.double()` while the float64 run is on; every input is converted to float64 beforehand (exact), so the whole
evaluation is a float64 one.  get_loss's own result is rcnn_loss = cls + (reg + corner); the reg-only gradient comes from the
reference's get_box_reg_layer_loss with CORNER_LOSS_REGULARIZATION switched off.

A second shim: current torch's F.binary_cross_entropy refuses targets outside [0, 1], and the reference hands it the ignored rows'
label -1 before it multiplies their (finite, log-clamped) element by the mask 0.  While the reference runs, the function gets those
targets as 0 instead; the elements concerned are exactly the ones the reference's mask zeroes, so no value or gradient it returns
depends on the replacement.

Stored per case: loss32 / loss64 = [rcnn_loss_cls, rcnn_loss_reg (as tb_dict logs it: before the corner term), rcnn_loss_corner (0 when absent),
rcnn_loss], tb32 / tb64 (the tb_dict as JSON), gcls{32,64} (n), greg / gtot {32,64} (fg rows x 7: d reg-only and d (reg + corner)
with respect to rcnn_reg; every non-fg row is asserted to be exactly 0), zeros: the packed bit mask of exact zeros of
[gcls64 | greg64 | gtot64] over all n rows.  Predictions: pred_{pv,pointrcnn}_{cls,reg} as int16 on the 1/64 grid.

Predictions lie on a 1/64 grid; logits include exactly 0 and +-20 (beyond +-27.6 the reference's clamps engage even in float64); the
planted zero row (roi == gt, rcnn_reg 0) has all eight corner distances and every regression difference exactly 0.  Asserted on the
reference alone, so that no element has to be left out of any comparison: no corner has |d - d_flip| < 1e-4, no corner distance
lies within 1e-4 of 1, no weighted regression difference lies within 1e-6 of 1/9.

Cases (tests/_roi_loss_torch.py:CASES)
  pv        roi_iou labels, corner term on, unit weights; frames 0, 1 (bg only), 3 of the pv case; zero row; headings moved by
            whole turns outside [-pi, pi]
  cls       the pointrcnn case's 1 / 0 / -1 labels
  weights   cls 2, reg 0.5, corner 0.25, code_weights [1, 0.5, 2, 0, 1.5, 1, 0.3]
  nocorner  CORNER_LOSS_REGULARIZATION off
  nofg      only the frame without a foreground roi
  ignored   every label -1
  nan       NaN gt columns (a centre, a size, the heading) on three fg rows

Usage:  python tests/golden/make_roi_loss_golden.py
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
import _roi_loss_torch as rlt  # noqa: E402

REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
PKG = "_refpcdet_rl"


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def load_reference():
    """-> (roi_head_template, loss_utils, box_coder_utils, box_utils) modules of the reference"""
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
    for sub in ["", ".utils", ".ops", ".ops.roiaware_pool3d", ".models", ".models.model_utils", ".models.roi_heads",
                ".models.roi_heads.target_assigner"]:
        pkg(PKG + sub, os.path.join(root, *sub.split(".")[1:]))
    sys.modules.setdefault("quaternion", types.ModuleType("quaternion"))
    for stub in [".ops.roiaware_pool3d.roiaware_pool3d_utils", ".models.model_utils.model_nms_utils",
                 ".models.roi_heads.target_assigner.proposal_target_layer"]:
        sys.modules[PKG + stub] = types.ModuleType(PKG + stub)
    sys.modules[PKG + ".models.model_utils.model_nms_utils"].class_agnostic_nms = None
    sys.modules[PKG + ".models.roi_heads.target_assigner.proposal_target_layer"].ProposalTargetLayer = None
    load(PKG + ".utils.common_utils", os.path.join(root, "utils", "common_utils.py"))
    box_utils = load(PKG + ".utils.box_utils", os.path.join(root, "utils", "box_utils.py"))
    coder = load(PKG + ".utils.box_coder_utils", os.path.join(root, "utils", "box_coder_utils.py"))
    loss_utils = load(PKG + ".utils.loss_utils", os.path.join(root, "utils", "loss_utils.py"))
    tmpl = load(PKG + ".models.roi_heads.roi_head_template", os.path.join(root, "models", "roi_heads", "roi_head_template.py"))
    return tmpl, loss_utils, coder, box_utils


def make_head(tmpl, coder, loss_cfg):
    h = tmpl.RoIHeadTemplate.__new__(tmpl.RoIHeadTemplate)
    nn.Module.__init__(h)
    h.model_cfg = Cfg(TARGET_CONFIG=Cfg(BOX_CODER="ResidualCoder"), LOSS_CONFIG=Cfg(loss_cfg))
    h.num_class = 3
    h.box_coder = coder.ResidualCoder()
    h.build_losses(h.model_cfg.LOSS_CONFIG)
    return h


def ret_dict(targets, cls, reg, dtype, grad):
    d = {}
    for k, v in targets.items():
        t = torch.from_numpy(np.array(v))
        d[k] = t.to(dtype) if t.is_floating_point() else t
    d["rcnn_cls"] = torch.from_numpy(cls.copy()).to(dtype).requires_grad_(grad)
    d["rcnn_reg"] = torch.from_numpy(reg.copy()).to(dtype).requires_grad_(grad)
    return d


def run(tmpl, coder, loss_cfg, targets, cls, reg, dtype, grad):
    """-> (losses (4), tb_dict, gradients or None) of the reference's get_loss"""
    head = make_head(tmpl, coder, loss_cfg)
    head.forward_ret_dict = ret_dict(targets, cls, reg, dtype, grad)
    with torch.set_grad_enabled(grad):
        loss, tb = head.get_loss()
    losses = np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0), tb["rcnn_loss"]], np.float64)
    if not grad:
        return losses, tb, None
    loss.backward()
    gcls = head.forward_ret_dict["rcnn_cls"].grad.numpy().copy()
    gtot = head.forward_ret_dict["rcnn_reg"].grad.numpy().copy()
    # reg only: the reference's own get_box_reg_layer_loss with the corner option off
    head = make_head(tmpl, coder, dict(loss_cfg, CORNER_LOSS_REGULARIZATION=False))
    head.forward_ret_dict = ret_dict(targets, cls, reg, dtype, True)
    reg_loss, _ = head.get_box_reg_layer_loss(head.forward_ret_dict)
    reg_loss.backward()
    greg = head.forward_ret_dict["rcnn_reg"].grad.numpy().copy()
    return losses, tb, (gcls, greg, gtot)


def check_clear_of_knees(coder, box_utils, loss_cfg, targets, reg):
    """the three assertions of the docstring, evaluated with the reference's own coder and corner function in float64"""
    fg = (targets["reg_valid_mask"] > 0).reshape(-1)
    if not fg.any():
        return
    t64 = lambda a: torch.from_numpy(np.array(a)).double()      # noqa: E731
    rois, gt, gs = (t64(targets[k]).reshape(fg.size, -1)[torch.from_numpy(fg)][:, :7] for k in ("rois", "gt_of_rois", "gt_of_rois_src"))
    pr = t64(reg)[torch.from_numpy(fg)]
    c = coder.ResidualCoder()
    anchor = rois.clone()
    anchor[:, 0:3] = 0
    anchor[:, 6] = 0
    tg = c.encode_torch(gt.clone(), anchor.clone())
    cw = torch.from_numpy(np.array(loss_cfg["LOSS_WEIGHTS"]["code_weights"], np.float32)).double()
    diff = ((pr - tg) * cw).abs()
    diff = diff[~torch.isnan(diff)]
    assert ((diff - 1.0 / 9.0).abs() >= 1e-6).all(), "a weighted regression difference within 1e-6 of 1/9"
    if not loss_cfg["CORNER_LOSS_REGULARIZATION"]:
        return
    anchor = rois.clone()
    anchor[:, 0:3] = 0
    box = c.decode_torch(pr, anchor)
    cr, sr = torch.cos(rois[:, 6]), torch.sin(rois[:, 6])
    x, y = box[:, 0] * cr - box[:, 1] * sr, box[:, 0] * sr + box[:, 1] * cr
    box = torch.cat([torch.stack([x, y, box[:, 2]], 1) + rois[:, 0:3], box[:, 3:]], 1)
    torch.Tensor.float, keep = torch.Tensor.double, torch.Tensor.float
    try:
        pc, gc = box_utils.boxes_to_corners_3d(box), box_utils.boxes_to_corners_3d(gs)
        flip = gs.clone()
        flip[:, 6] += np.pi
        fc = box_utils.boxes_to_corners_3d(flip)
    finally:
        torch.Tensor.float = keep
    da, db = torch.norm(pc - gc, dim=2), torch.norm(pc - fc, dim=2)
    assert ((da - db).abs() >= 1e-4).all(), "a corner with |d - d_flip| < 1e-4"
    d = torch.minimum(da, db)
    assert ((d - 1.0).abs() >= 1e-4).all(), "a corner distance within 1e-4 of 1"
    print(f"      corner distances: {int((d < 1).sum())} below 1, {int((d >= 1).sum())} above, {int((db < da).sum())} flipped, "
          f"{int((d == 0).sum())} exactly 0")


def predictions(seed, ptz):
    """int16 grid values (x 1/64) per base case: logits N(0, 3) with planted 0 and +-20, regressions near 0"""
    r = np.random.default_rng(seed)
    out = {}
    for base in ("pv", "pointrcnn"):
        B, P = ptz[f"{base}_out_reg_valid_mask"].shape
        cls = np.round(r.normal(0, 3, (B, P)) * 64).clip(-1280, 1280)
        cls[:, 5], cls[:, 17], cls[:, 40], cls[:, 70], cls[:, 100] = 0, 1280, -1280, 1280, 0
        scale = np.array([0.3, 0.3, 0.3, 0.15, 0.15, 0.15, 0.25])
        reg = np.round(r.normal(0, 1, (B, P, 7)) * scale * 64)
        out[f"pred_{base}_cls"], out[f"pred_{base}_reg"] = cls.astype(np.int16), reg.astype(np.int16)
    fg0 = np.nonzero(ptz["pv_out_reg_valid_mask"][0] > 0)[0][0]         # the planted zero row of the cases that start at pv frame 0
    out["pred_pv_reg"][0, fg0] = 0
    return out


def main():
    tmpl, _loss_utils, coder, box_utils = load_reference()
    ptz = np.load(os.path.join(HERE, "proposal_target_ref.npz"))
    cuda, flt, bce = torch.Tensor.cuda, torch.Tensor.float, torch.nn.functional.binary_cross_entropy
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.functional.binary_cross_entropy = lambda x, t, *a, **k: bce(x, torch.where(t < 0, torch.zeros_like(t), t), *a, **k)
    try:
        for seed in range(300, 340):
            out = predictions(seed, ptz)
            try:
                for name, (_base, _frames, cfg, _plants) in rlt.CASES.items():
                    targets = rlt.case_targets(name, ptz)
                    cls, reg = rlt.case_predictions(name, out)
                    print(f"   {name}: n {cls.shape[0]}, fg {int((targets['reg_valid_mask'] > 0).sum())}, valid "
                          f"{int((targets['rcnn_cls_labels'] >= 0).sum())}")
                    check_clear_of_knees(coder, box_utils, cfg, targets, reg)
                    l32, tb32, _ = run(tmpl, coder, cfg, targets, cls, reg, torch.float32, False)
                    l32g, _, g32 = run(tmpl, coder, cfg, targets, cls, reg, torch.float32, True)
                    assert np.array_equal(l32, l32g), "the float32 run changes under autograd"
                    torch.Tensor.float = torch.Tensor.double
                    try:
                        l64, tb64, g64 = run(tmpl, coder, cfg, targets, cls, reg, torch.float64, True)
                    finally:
                        torch.Tensor.float = flt
                    fg = (targets["reg_valid_mask"] > 0).reshape(-1)
                    for g in (*g32[1:], *g64[1:]):
                        assert not g[~fg].any(), "a non-fg row with a regression gradient"
                    out[f"{name}_loss32"], out[f"{name}_loss64"] = l32, l64
                    out[f"{name}_tb32"], out[f"{name}_tb64"] = np.array(json.dumps(tb32)), np.array(json.dumps(tb64))
                    for tag, (gc, gr, gt) in (("32", g32), ("64", g64)):
                        out[f"{name}_gcls{tag}"], out[f"{name}_greg{tag}"], out[f"{name}_gtot{tag}"] = gc.reshape(-1), gr[fg], gt[fg]
                    out[f"{name}_zeros"] = np.packbits(np.concatenate([g.reshape(-1) == 0 for g in g64]))
                    z = rlt.zero_row(name, targets)
                    if z is not None:
                        assert not g64[1][z].any() and not g64[2][z].any() and np.isfinite(g64[2]).all(), "the planted zero row"
                    print(f"      float32 {l32.tolist()}\n      float64 {l64.tolist()}")
                break
            except AssertionError as e:
                print(f"   seed {seed}: {e}")
        else:
            raise RuntimeError("no seed keeps the fixture clear of the knees")
    finally:
        torch.Tensor.cuda, torch.Tensor.float, torch.nn.functional.binary_cross_entropy = cuda, flt, bce
    out["cases"] = np.array(json.dumps({k: dict(base=v[0], frames=v[1], loss_config=v[2], plants=list(v[3])) for k, v in rlt.CASES.items()}))
    path = os.path.join(HERE, "roi_loss_ref.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(HERE, "proposal_target_ref.npz"))
    print(path, os.path.getsize(path), "bytes; proposal_target_ref.npz", limit)
    assert os.path.getsize(path) <= limit


if __name__ == "__main__":
    main()
