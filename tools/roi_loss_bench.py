"""Times the RoI-head loss at PV-RCNN's training shape (bs 8, ROI_PER_IMAGE 128, pv_rcnn.yaml's LOSS_CONFIG): the fused forward +
backward (lidardetection_amd/roi_loss.py) against `ported_get_loss` below, a torch port of the reference's
RoIHeadTemplate.get_loss (fg_sum read back with .item(), three boolean-mask gathers, one .item() per logged value), forward +
backward, on the same tensors in the same process.  The port exists only for this comparison.

Reports per column: wall time per call (device events, median after warm-up), host time to enqueue without a final
synchronisation (the port synchronises inside, so its enqueue time is its wall time), the number of device kernels and of
device-to-host copies and .item() calls (torch.profiler).  Also the forward alone and the mirror's get_loss (one copy).  Prints one JSON line.

  python tools/roi_loss_bench.py [--iters 200] [--ref-iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidardetection_amd import roi_loss  # noqa: E402
from lidardetection_amd.pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate, _corners, _smooth_l1  # noqa: E402
from lidardetection_amd.pcdet.utils.cfg import AttrDict  # noqa: E402
from lidardetection_amd.pvrcnn import LOSS_CONFIG, TARGET_CONFIG  # noqa: E402

from _measure import enqueue_ms, event_ms, kernel_count  # noqa: E402


def ported_get_loss(d, lw):
    """the reference's get_loss, step for step (roi_head_template.py:133-233), except that the inputs are not clamped in place"""
    tb = {}
    x, t = d["rcnn_cls"].view(-1), d["rcnn_cls_labels"].view(-1)
    each = F.binary_cross_entropy(torch.sigmoid(x), torch.clamp(t, min=0.0), reduction="none")
    valid = (t >= 0).float()
    cls = (each * valid).sum() / torch.clamp(valid.sum(), min=1.0) * lw["rcnn_cls_weight"]
    tb["rcnn_loss_cls"] = cls.item()
    n = x.shape[0]
    fg = d["reg_valid_mask"].view(-1) > 0
    fg_sum = fg.long().sum().item()
    roi, gt, reg = d["rois"].view(n, 7), d["gt_of_rois"].view(n, 8)[:, :7], d["rcnn_reg"]
    da, dg = torch.clamp_min(roi[:, 3:6], 1e-5), torch.clamp_min(gt[:, 3:6], 1e-5)
    diag = torch.sqrt(da[:, 0:1] ** 2 + da[:, 1:2] ** 2)
    tg = torch.cat([gt[:, 0:2] / diag, gt[:, 2:3] / da[:, 2:3], torch.log(dg / da), gt[:, 6:7]], dim=-1)
    tg = torch.where(torch.isnan(tg), reg, tg)
    diff = (reg - tg) * reg.new_tensor(lw["code_weights"]).view(1, -1)
    loss_reg = (_smooth_l1(diff.abs(), 1.0 / 9.0) * fg.unsqueeze(-1).float()).sum() / max(fg_sum, 1) * lw["rcnn_reg_weight"]
    tb["rcnn_loss_reg"] = loss_reg.item()
    if fg_sum > 0:
        p, r = reg[fg], roi[fg]
        dg_ = torch.sqrt(r[:, 3] ** 2 + r[:, 4] ** 2)
        xl, yl = p[:, 0] * dg_, p[:, 1] * dg_
        c, s = torch.cos(r[:, 6]), torch.sin(r[:, 6])
        box = torch.stack([xl * c - yl * s + r[:, 0], xl * s + yl * c + r[:, 1], p[:, 2] * r[:, 5] + r[:, 2], torch.exp(p[:, 3]) * r[:, 3],
                           torch.exp(p[:, 4]) * r[:, 4], torch.exp(p[:, 5]) * r[:, 5], p[:, 6] + r[:, 6]], dim=1)
        gs = d["gt_of_rois_src"].view(n, 8)[fg][:, :7]
        flip = gs.clone()
        flip[:, 6] += np.pi
        pc = _corners(box)
        dist = torch.min(torch.norm(pc - _corners(gs), dim=2), torch.norm(pc - _corners(flip), dim=2))
        corner = _smooth_l1(dist, 1.0).mean(dim=1).mean() * lw["rcnn_corner_weight"]
        loss_reg = loss_reg + corner
        tb["rcnn_loss_corner"] = corner.item()
    loss = cls + loss_reg
    tb["rcnn_loss"] = loss.item()
    return loss, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ref-iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("roi_loss_bench: no GPU")
    dev = torch.device("cuda:0")
    B, P = 8, TARGET_CONFIG["ROI_PER_IMAGE"]
    n = B * P
    g = torch.Generator().manual_seed(7)
    u = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    rois = torch.cat([u(n, 2) * 70, u(n, 1) * 2 - 2, 1 + u(n, 3) * 3, u(n, 1) * 6 - 3], 1)
    src = torch.cat([rois[:, :3] + (u(n, 3) - 0.5), rois[:, 3:6] * (0.8 + 0.4 * u(n, 3)), rois[:, 6:7] + (u(n, 1) - 0.5) * 0.6, u(n, 1)], 1)
    gt = torch.cat([u(n, 3) - 0.5, src[:, 3:6], (u(n, 1) - 0.5) * 0.6, src[:, 7:8]], 1)
    d = dict(rois=rois.view(B, P, 7), gt_of_rois=gt.view(B, P, 8), gt_of_rois_src=src.view(B, P, 8),
             reg_valid_mask=(u(B, P) < 0.4).long(), rcnn_cls_labels=u(B, P))
    d = {k: v.contiguous().to(dev) for k, v in d.items()}
    x = (torch.randn(n, 1, generator=g) * 2).to(dev).requires_grad_(True)
    r = (torch.randn(n, 7, generator=g) * 0.15).to(dev).requires_grad_(True)
    spec = roi_loss.spec_from_cfg(dict(LOSS_CONFIG=LOSS_CONFIG))
    lw = LOSS_CONFIG["LOSS_WEIGHTS"]
    head = RoIHeadTemplate(3, AttrDict(TARGET_CONFIG=AttrDict(TARGET_CONFIG), LOSS_CONFIG=AttrDict(LOSS_CONFIG)))

    def fused():
        x.grad = r.grad = None
        cls, reg, cor, _ = roi_loss.roi_head_loss(x, r, d, spec)
        (cls + reg + cor).backward()

    def fused_forward():
        with torch.no_grad():
            roi_loss.roi_head_loss(x, r, d, spec)

    def mirror_get_loss():
        head.forward_ret_dict = dict(d, rcnn_cls=x, rcnn_reg=r)
        with torch.no_grad():
            head.get_loss()

    def port():
        x.grad = r.grad = None
        loss, _ = ported_get_loss(dict(d, rcnn_cls=x, rcnn_reg=r), lw)
        loss.backward()

    result = {"tool": "roi_loss_bench", "device": torch.cuda.get_device_name(0), "batch": B, "roi_per_image": P,
              "fg_rows": int(d["reg_valid_mask"].sum())}
    for name, fn, iters in [("fused_fwd_bwd", fused, args.iters), ("fused_forward", fused_forward, args.iters),
                            ("mirror_get_loss", mirror_get_loss, args.iters), ("torch_port_fwd_bwd", port, args.ref_iters)]:
        med, lo, _ = event_ms(fn, iters, 10)
        k = kernel_count(fn)
        result[name] = {"wall_ms_median": round(med, 4), "wall_ms_min": round(lo, 4), "enqueue_ms": round(enqueue_ms(fn, iters), 4),
                        "device_kernels": k["kernels"], "device_to_host_copies": k["d2h_copies"], "item_calls": k["item_calls"]}
        if name != "torch_port_fwd_bwd":
            result[name]["kernel_names"] = k["names"]
    result["speedup_wall"] = round(result["torch_port_fwd_bwd"]["wall_ms_median"] / result["fused_fwd_bwd"]["wall_ms_median"], 1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
