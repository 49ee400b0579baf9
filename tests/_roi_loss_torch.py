"""A torch restatement of the RoI-head loss (RoIHeadTemplate.get_loss of the reference with CLS_LOSS BinaryCrossEntropy, REG_LOSS
smooth-l1 and the corner regulariser) in this project's words, in whatever dtype and on whatever device its inputs have.
tests/test_roi_loss_host.py pins it in float64 to the reference's own float64 run (tests/golden/roi_loss_ref.npz); that agreement is
what licenses it as the oracle of the raw-ABI sweep in tests/test_gpu_roi_loss.py.

Differences from the reference's text, none of which changes a value on the fixture: BCE in the stable logit form (equal for
|x| < 27.6), fg rows gathered once, the flipped gt's corners formed by negating the unflipped x / y offsets, nothing written in
place."""
import math

import torch

SIGNS = [(1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1)]   # boxes_to_corners_3d


def smooth_l1(n, beta):
    return torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def corners(box):
    """(m, 7) -> (m, 8, 3)"""
    t = torch.tensor(SIGNS, dtype=box.dtype, device=box.device) / 2
    off = box[:, None, 3:6] * t[None]
    c, s = torch.cos(box[:, 6])[:, None], torch.sin(box[:, 6])[:, None]
    x = off[..., 0] * c - off[..., 1] * s
    y = off[..., 0] * s + off[..., 1] * c
    return torch.stack([x, y, off[..., 2]], dim=-1) + box[:, None, 0:3]


def roi_loss(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask, rcnn_cls_labels, weights, code_weights, corner):
    """-> (cls, reg, corner) 0-dim tensors, (fg_sum, n_valid) tensors.  weights (cls, reg, corner); code_weights 7 floats (taken as
    float32 values, as the reference stores them)."""
    dt, dev = rcnn_reg.dtype, rcnn_reg.device
    n = rcnn_reg.shape[0]
    x, t = rcnn_cls.reshape(n), rcnn_cls_labels.reshape(n).to(dt)
    valid = t >= 0
    # BCE with logits as -t log sigmoid(x) - (1 - t) log sigmoid(-x): stable, and autograd's gradient is sigmoid(x) - t at x == 0 too
    # (max(x, 0) - x t + log1p(exp(-|x|)) is the same value, but autograd's subgradients of max and abs at 0 give 1 - t there)
    bce = -t * torch.nn.functional.logsigmoid(x) - (1 - t) * torch.nn.functional.logsigmoid(-x)
    n_valid = valid.sum()
    cls = torch.where(valid, bce, torch.zeros_like(bce)).sum() / torch.clamp(n_valid.to(dt), min=1.0) * weights[0]

    fg = reg_valid_mask.reshape(n) > 0
    fg_sum = fg.sum()
    pr = rcnn_reg[fg]
    roi = rois.reshape(n, -1)[fg][:, :7].to(dt)
    g = gt_of_rois.reshape(n, -1)[fg][:, :7].to(dt)
    gs = gt_of_rois_src.reshape(n, -1)[fg][:, :7].to(dt)
    cw = torch.tensor([float(torch.tensor(w, dtype=torch.float32)) for w in code_weights], dtype=dt, device=dev)
    da, dg = torch.clamp_min(roi[:, 3:6], 1e-5), torch.clamp_min(g[:, 3:6], 1e-5)
    diag = torch.sqrt(da[:, 0] ** 2 + da[:, 1] ** 2)
    tg = torch.stack([g[:, 0] / diag, g[:, 1] / diag, g[:, 2] / da[:, 2], torch.log(dg[:, 0] / da[:, 0]), torch.log(dg[:, 1] / da[:, 1]),
                      torch.log(dg[:, 2] / da[:, 2]), g[:, 6]], dim=1)
    tg = torch.where(torch.isnan(tg), pr, tg)                                    # a NaN target takes the prediction: difference 0
    diff = (pr - tg) * cw
    denom = torch.clamp(fg_sum.to(dt), min=1.0)
    reg = smooth_l1(diff.abs(), 1.0 / 9.0).sum() / denom * weights[1]

    cor = torch.zeros((), dtype=dt, device=dev)
    if corner:
        diag_r = torch.sqrt(roi[:, 3] ** 2 + roi[:, 4] ** 2)
        xl, yl, zl = pr[:, 0] * diag_r, pr[:, 1] * diag_r, pr[:, 2] * roi[:, 5]
        c, s = torch.cos(roi[:, 6]), torch.sin(roi[:, 6])
        pred = torch.stack([xl * c - yl * s, xl * s + yl * c, zl, torch.exp(pr[:, 3]) * roi[:, 3], torch.exp(pr[:, 4]) * roi[:, 4],
                            torch.exp(pr[:, 5]) * roi[:, 5], pr[:, 6] + roi[:, 6]], dim=1)
        gl = torch.cat([gs[:, 0:3] - roi[:, 0:3], gs[:, 3:7]], dim=1)          # the roi centre goes to the gt side
        pc, gc = corners(pred), corners(gl)
        flip = torch.cat([2 * gl[:, None, 0:2] - gc[..., 0:2], gc[..., 2:3]], dim=-1)      # the gt turned by pi about its centre
        d2a, d2b = ((pc - gc) ** 2).sum(-1), ((pc - flip) ** 2).sum(-1)
        d2 = torch.minimum(d2a, d2b)
        safe = torch.where(d2 > 0, d2, torch.ones_like(d2))
        dist = torch.where(d2 > 0, torch.sqrt(safe), torch.zeros_like(d2))       # gradient 0 at distance 0, as torch.norm's
        cor = smooth_l1(dist, 1.0).mean(dim=1).sum() / denom * weights[2]
    return (cls, reg, cor), (fg_sum, n_valid)


def case_weights(cfg):
    """(weights, code_weights, corner) of a fixture case's LOSS_CONFIG dict"""
    lw = cfg["LOSS_WEIGHTS"]
    corner = bool(cfg.get("CORNER_LOSS_REGULARIZATION", False))
    return ((lw["rcnn_cls_weight"], lw["rcnn_reg_weight"], lw["rcnn_corner_weight"] if corner else 0.0), lw["code_weights"], corner)


# ---------------------------------------------------------------- the fixture's cases (tests/golden/make_roi_loss_golden.py)
PV_LOSS = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
               LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7))
WEIGHTED = dict(PV_LOSS, LOSS_WEIGHTS=dict(rcnn_cls_weight=2.0, rcnn_reg_weight=0.5, rcnn_corner_weight=0.25,
                                           code_weights=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.3]))
# name -> (case of proposal_target_ref.npz, its frames, LOSS_CONFIG, planted changes)
CASES = {
    "pv": ("pv", [0, 1, 3], PV_LOSS, ("zero_row", "headings")),
    "cls": ("pointrcnn", [0, 1], PV_LOSS, ()),
    "weights": ("pv", [0, 3], WEIGHTED, ("zero_row",)),
    "nocorner": ("pv", [3], dict(PV_LOSS, CORNER_LOSS_REGULARIZATION=False), ()),
    "nofg": ("pv", [1], PV_LOSS, ()),
    "ignored": ("pv", [3], PV_LOSS, ("ignored",)),
    "nan": ("pv", [3], PV_LOSS, ("nan",)),
}
TARGET_KEYS = ("rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels")


def case_targets(name, ptz):
    """the targets_dict of a case as numpy arrays: the frames of the reference's ProposalTargetLayer + assign_targets output stored
    in proposal_target_ref.npz (`ptz`), with the case's planted values.  The loss takes the five tensors as independent inputs, so a
    planted row need not be what assign_targets would derive."""
    import numpy as np
    base, frames, _cfg, plants = CASES[name]
    t = {k: np.array(ptz[f"{base}_out_{k}"][frames]) for k in TARGET_KEYS}
    t["rcnn_cls_labels"] = t["rcnn_cls_labels"].astype(np.float32)           # CLS_SCORE_TYPE cls: the reference returns int64
    fg = np.argwhere(t["reg_valid_mask"] > 0)
    if "zero_row" in plants:         # a roi equal to its gt (its prediction is planted as 0): every difference is exactly 0
        b, i = fg[0]
        t["gt_of_rois_src"][b, i, :7] = t["rois"][b, i]
        t["gt_of_rois"][b, i, :7] = [0, 0, 0, *t["rois"][b, i, 3:6], 0]
    if "headings" in plants:         # headings outside [-pi, pi] on both sides of the corner term
        for (b, i), turns in zip(fg[1:4], (2, -1, 3)):
            t["rois"][b, i, 6] += np.float32(turns * 2 * math.pi)
            t["gt_of_rois_src"][b, i, 6] -= np.float32(turns * 2 * math.pi)
    if "ignored" in plants:
        t["rcnn_cls_labels"][:] = -1.0
    if "nan" in plants:              # NaN columns of the canonical gt on fg rows: a centre, a size and the heading
        for (b, i), col in zip(fg[:3], (0, 4, 6)):
            t["gt_of_rois"][b, i, col] = np.nan
    return t


def zero_row(name, targets):
    """flat index of the planted zero row, or None"""
    import numpy as np
    if "zero_row" not in CASES[name][3]:
        return None
    b, i = np.argwhere(targets["reg_valid_mask"] > 0)[0]
    return int(b * targets["reg_valid_mask"].shape[1] + i)


def case_predictions(name, rz):
    """(rcnn_cls (n, 1), rcnn_reg (n, 7)) float32 of a case: stored as integers on the 1/64 grid"""
    import numpy as np
    base, frames, _cfg, _plants = CASES[name]
    P = rz[f"pred_{base}_cls"].shape[1]
    cls = rz[f"pred_{base}_cls"][frames].reshape(len(frames) * P, 1).astype(np.float32) / 64
    reg = rz[f"pred_{base}_reg"][frames].reshape(len(frames) * P, 7).astype(np.float32) / 64
    return cls, reg


def fixture_grads(name, rz, run, targets):
    """the reference's gradients of a case -> (d cls / d rcnn_cls (n, 1), d reg / d rcnn_reg, d (reg + corner) / d rcnn_reg (n, 7))
    float64 arrays; the file keeps the fg rows of the latter two (the generator asserts that every other row is exactly 0)"""
    import numpy as np
    fg = (targets["reg_valid_mask"] > 0).reshape(-1)
    out = [np.asarray(rz[f"{name}_gcls{run}"], np.float64).reshape(-1, 1)]
    for k in ("greg", "gtot"):
        g = np.zeros((fg.size, 7), np.float64)
        g[fg] = rz[f"{name}_{k}{run}"]
        out.append(g)
    return out
