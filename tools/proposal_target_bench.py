"""Times second-stage target assignment at PV-RCNN's training shape (bs 8, 512 rois, 40 gt rows, three classes, pv_rcnn.yaml's
TARGET_CONFIG): the one-launch HIP call (RoIHeadTemplate.assign_targets of this package) against `looped_assign` below, a torch
port of the reference's host loop (per frame: trim by reading row sums back, per class a boxes_iou3d_gpu call on this package's
kernels, nonzero() per category, numpy / torch.randint sampling on the host; then the canonical transform as tensor ops) on the
same GPU.  The port exists only for this comparison.

Reports per call: wall time (device events, the call alone on an idle stream), host time to enqueue without a final
synchronisation (the looped port synchronises inside, so its enqueue time is its wall time), and the number of device kernels
(torch.profiler).  Prints one JSON line.

  python tools/proposal_target_bench.py [--iters 200] [--ref-iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidardetection_amd import synth  # noqa: E402
from lidardetection_amd.pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate  # noqa: E402
from lidardetection_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils  # noqa: E402
from lidardetection_amd.pcdet.utils import common_utils  # noqa: E402
from lidardetection_amd.pcdet.utils.cfg import AttrDict  # noqa: E402
from lidardetection_amd.pvrcnn import TARGET_CONFIG  # noqa: E402

from _measure import enqueue_ms, event_ms, kernel_count  # noqa: E402


def looped_assign(cfg, rois, roi_scores, roi_labels, gt_boxes):
    """the reference's ProposalTargetLayer + assign_targets as a host loop over frames and classes (by class, roi_iou)"""
    B, P = rois.shape[0], cfg.ROI_PER_IMAGE
    o_rois, o_gt = rois.new_zeros(B, P, rois.shape[-1]), rois.new_zeros(B, P, gt_boxes.shape[-1])
    o_iou, o_scores = rois.new_zeros(B, P), rois.new_zeros(B, P)
    o_labels = rois.new_zeros((B, P), dtype=torch.long)
    fg_quota = int(np.round(cfg.FG_RATIO * P))
    fg_thresh = min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)

    def draw(cands, n):
        return cands[torch.randint(low=0, high=cands.numel(), size=(n,)).long().to(cands.device)]

    for b in range(B):
        gt = gt_boxes[b]
        k = len(gt) - 1
        while k > 0 and gt[k].sum() == 0:                     # one device read per step
            k -= 1
        gt = gt[:k + 1]
        gl = gt[:, -1].long()
        ov, asg = rois.new_zeros(rois.shape[1]), roi_labels.new_zeros(rois.shape[1])
        for c in range(gl.min().item(), gl.max().item() + 1):
            rm, gm = roi_labels[b] == c, gl == c
            if rm.sum() > 0 and gm.sum() > 0:
                iou = iou3d_nms_utils.boxes_iou3d_gpu(rois[b][rm][:, :7], gt[gm][:, :7])
                best, arg = torch.max(iou, dim=1)
                ov[rm] = best
                asg[rm] = gm.nonzero().view(-1)[arg]
        fg = (ov >= fg_thresh).nonzero().view(-1)
        easy = (ov < cfg.CLS_BG_THRESH_LO).nonzero().view(-1)
        hard = ((ov < cfg.REG_FG_THRESH) & (ov >= cfg.CLS_BG_THRESH_LO)).nonzero().view(-1)
        n_bg = hard.numel() + easy.numel()
        if fg.numel() > 0 and n_bg > 0:
            n_fg = min(fg_quota, fg.numel())
            picks = [fg[torch.from_numpy(np.random.permutation(fg.numel())).to(fg.device)[:n_fg]]]
        elif fg.numel() > 0:
            n_fg = P
            picks = [fg[torch.from_numpy(np.floor(np.random.rand(P) * fg.numel())).long().to(fg.device)]]
        else:
            n_fg, picks = 0, []
        n = P - n_fg
        if n > 0:
            if hard.numel() > 0 and easy.numel() > 0:
                n_hard = min(int(n * cfg.HARD_BG_RATIO), hard.numel())
                picks += [draw(hard, n_hard), draw(easy, n - n_hard)]
            else:
                picks.append(draw(hard if hard.numel() > 0 else easy, n))
        idx = torch.cat(picks)
        o_rois[b], o_labels[b], o_iou[b], o_scores[b] = rois[b][idx], roi_labels[b][idx], ov[idx], roi_scores[b][idx]
        o_gt[b] = gt[asg[idx]]
    reg_valid = (o_iou > cfg.REG_FG_THRESH).long()
    fg_mask, bg_mask = o_iou > cfg.CLS_FG_THRESH, o_iou < cfg.CLS_BG_THRESH
    mid = (fg_mask == 0) & (bg_mask == 0)
    cls = (fg_mask > 0).float()
    cls[mid] = (o_iou[mid] - cfg.CLS_BG_THRESH) / (cfg.CLS_FG_THRESH - cfg.CLS_BG_THRESH)
    src = o_gt.clone()
    ry = o_rois[:, :, 6] % (2 * np.pi)
    o_gt[:, :, 0:3] = o_gt[:, :, 0:3] - o_rois[:, :, 0:3]
    o_gt[:, :, 6] = o_gt[:, :, 6] - ry
    o_gt = common_utils.rotate_points_along_z(o_gt.view(-1, 1, o_gt.shape[-1]), -ry.view(-1)).view(B, -1, o_gt.shape[-1])
    h = o_gt[:, :, 6] % (2 * np.pi)
    opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h[opp] = (h[opp] + np.pi) % (2 * np.pi)
    h[h > np.pi] -= np.pi * 2
    o_gt[:, :, 6] = torch.clamp(h, min=-np.pi / 2, max=np.pi / 2)
    return {"rois": o_rois, "gt_of_rois": o_gt, "gt_of_rois_src": src, "gt_iou_of_rois": o_iou, "roi_scores": o_scores,
            "roi_labels": o_labels, "reg_valid_mask": reg_valid, "rcnn_cls_labels": cls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ref-iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("proposal_target_bench: no GPU")
    dev = torch.device("cuda:0")
    cfg = AttrDict(TARGET_CONFIG)
    rois, scores, labels, gt = (torch.from_numpy(x).to(dev) for x in synth.rcnn_target_inputs(5000, batch=8, rois=512, max_gt=40))
    head = RoIHeadTemplate(3, AttrDict(TARGET_CONFIG=cfg))
    batch = {"batch_size": 8, "rois": rois, "roi_scores": scores, "roi_labels": labels, "gt_boxes": gt}
    fg_keys, draws = head.proposal_target_layer.random_inputs(rois)
    hip = lambda: head.assign_targets(batch)                                      # noqa: E731  draws its random numbers itself
    hip_fixed = lambda: head.assign_targets(batch, fg_keys=fg_keys, draws=draws)  # noqa: E731  the launch alone
    port = lambda: looped_assign(cfg, rois, scores, labels, gt)                   # noqa: E731
    result = {"tool": "proposal_target_bench", "device": torch.cuda.get_device_name(0), "batch": 8, "rois": 512, "max_gt": 40,
              "roi_per_image": cfg.ROI_PER_IMAGE}
    for name, fn, iters in [("hip", hip, args.iters), ("hip_given_random_numbers", hip_fixed, args.iters), ("looped_port", port, args.ref_iters)]:
        med, lo, _ = event_ms(fn, iters, 5)
        k = kernel_count(fn)
        result[name] = {"wall_ms_median": round(med, 4), "wall_ms_min": round(lo, 4), "enqueue_ms": round(enqueue_ms(fn, iters), 4),
                        "device_kernels": k["kernels"], "device_copies": k["copies"]}
        if name != "looped_port":
            result[name]["kernel_names"] = k["names"]
    result["speedup_wall"] = round(result["looped_port"]["wall_ms_median"] / result["hip"]["wall_ms_median"], 1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
