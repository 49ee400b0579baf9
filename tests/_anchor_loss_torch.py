"""What the anchor-head loss tests (tests/test_anchor_loss_host.py, tests/test_gpu_anchor_loss.py) and tools/loss_bench.py share:
the reference fixture's loader (tests/golden/anchor_loss_ref.npz, written by tests/golden/make_loss_golden.py), `restated_loss` —
a torch restatement of the reference's RPN loss written for these tests, which tests/test_anchor_loss_host.py pins to the
reference's own fp64 losses and autograd gradients — and the two production-size workloads (labels and targets from the GPU
assigner)."""
import json
import math
import os

import numpy as np
import torch

from lidardetection_amd import anchor_loss
from lidardetection_amd.pcdet.utils.cfg import AttrDict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss_ref.npz")
CASES = ["kitti", "agnostic", "nodir", "kitti_multi", "nus", "multi_nosep"]
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ torch restatement
def direction_bins(targets, anchors, dir_offset, num_bins):
    """the direction class of every anchor, in fp32 on the targets' device; divisions by fp32 tensors (true division on every
    device, as torch's CPU kernels divide by a Python scalar)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=targets.device)   # noqa: E731
    rot = targets[..., 6].float() + anchors[:, 6].float().unsqueeze(0)
    v = rot - f(dir_offset)
    two_pi = f(2 * math.pi)
    r = v - torch.floor(v / two_pi) * two_pi
    return torch.floor(r / f(2 * math.pi / num_bins)).long().clamp(0, num_bins - 1)


def restated_loss(cls, box, dirs, labels, targets, anchors, spec):
    """(cls_loss, loc_loss, dir_loss) of the reference's RPN loss, differentiable.  cls / box / dirs: per-head (B, n_h, c) tensors
    in the heads' anchor order (dirs may be empty); labels (B, N) int; targets (B, N, code) and anchors (N, D) fp32."""
    dt = box[0].dtype
    B, N = labels.shape
    lab = labels.long()
    if spec.num_class == 1:
        lab = torch.where(lab > 0, torch.ones_like(lab), lab)
    pos, neg = lab > 0, lab == 0
    # the class and box weights are fp32 tensors whatever the predictions' dtype; the direction weights take the logits' dtype
    norm32 = pos.sum(1, keepdim=True).float().clamp(min=1.0)
    norm = pos.sum(1, keepdim=True).to(dt).clamp(min=1.0)
    cls_w = ((pos.float() * spec.pos_cls_weight + neg.float() * spec.neg_cls_weight) / norm32).to(dt)
    onehot = torch.nn.functional.one_hot(lab.clamp(min=0), spec.num_class + 1)[..., 1:].to(dt)
    sep = spec.multihead and spec.separate
    sin_diff = not spec.multihead or len(dirs) > 0
    cw = torch.tensor(spec.code_weights, dtype=torch.float32, device=labels.device).to(dt)   # an fp32 buffer in the reference
    bins = direction_bins(targets, anchors, spec.dir_offset, spec.num_dir_bins) if dirs else None
    lc = ll = ld = 0.0
    a0 = 0
    for h, x in enumerate(cls):
        n = x.shape[1]
        c0 = spec.head_class_offsets[h] if sep else 0
        t = onehot[:, a0:a0 + n, c0:c0 + x.shape[2]]
        p = torch.sigmoid(x)
        focal = torch.where(t > 0, 0.25 * (1.0 - p) ** 2, 0.75 * p ** 2)
        bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
        lc = lc + (focal * bce * cls_w[:, a0:a0 + n, None]).sum()
        w = (pos[:, a0:a0 + n].float() / norm32).to(dt)
        pb, t32 = box[h], targets[:, a0:a0 + n]
        tg = t32.to(dt)
        if sin_diff:   # the target's sin / cos in the targets' fp32, the prediction's in its own dtype
            s = torch.sin(pb[..., 6:7]) * torch.cos(t32[..., 6:7]).to(dt)
            c = torch.cos(pb[..., 6:7]) * torch.sin(t32[..., 6:7]).to(dt)
            pb = torch.cat([pb[..., :6], s, pb[..., 7:]], dim=-1)
            tg = torch.cat([tg[..., :6], c, tg[..., 7:]], dim=-1)
        tg = torch.where(torch.isnan(tg), pb, tg)
        d = ((pb - tg) * cw).abs()
        if spec.reg_loss == "WeightedSmoothL1Loss":
            beta = 1.0 / 9.0 if dt == torch.float64 else torch.tensor(1.0 / 9.0, dtype=dt).item()
            d = torch.where(d < beta, 0.5 * d ** 2 / beta, d - 0.5 * beta)
        ll = ll + (d * w[..., None]).sum()
        if dirs:
            logp = torch.log_softmax(dirs[h], dim=-1)
            ce = -logp.gather(-1, bins[:, a0:a0 + n, None]).squeeze(-1)
            ld = ld + (ce * (pos[:, a0:a0 + n].to(dt) / norm)).sum()
        a0 += n
    zero = box[0].new_zeros(())
    return (lc / B * spec.cls_weight, ll / B * spec.loc_weight, (ld / B * spec.dir_weight) if dirs else zero)


def load_case(name):
    z = np.load(GOLDEN)
    meta = json.loads(str(z[f"{name}_meta"]))
    get = lambda short: [torch.from_numpy(z[f"{name}_{short}_{k}"]) for k in range(32) if f"{name}_{short}_{k}" in z]  # noqa: E731
    preds = {s: get(s) for s in ["cls", "box", "dir"]}
    grads = {s: get("g" + s) for s in ["cls", "box", "dir"]}
    # the exact zeros of the fp64 gradients, unpacked to the gradients' shapes
    zeros = {s: [torch.from_numpy(np.unpackbits(z[f"{name}_z{s}_{k}"])[:g.numel()].astype(bool)).reshape(g.shape)
                 for k, g in enumerate(grads[s])] for s in ["cls", "box", "dir"]}
    grads["zero"] = zeros
    arr = {k: torch.from_numpy(z[f"{name}_{k}"]) for k in ["labels", "labels_after", "targets", "anchors", "gt", "loss32", "loss64"]}
    return meta, preds, grads, arr


def spec_of(meta):
    return anchor_loss.spec_from_cfg(AttrDict(meta["model_cfg"]), meta["num_class"],
                                     meta["head_num_classes"] if meta["kind"] == "multi" else None)


def per_head(meta, preds, B):
    """the fixture's predictions in the reference's views -> per-head (B, n_h, c) tensors"""
    spec = spec_of(meta)
    code = meta["code_size"]
    cols = list(spec.head_classes) if meta["kind"] == "multi" and spec.separate else [spec.num_class] * len(preds["cls"])
    cls = [x.reshape(B, -1, c) for x, c in zip(preds["cls"], cols)]
    box = [x.reshape(B, -1, code) for x in preds["box"]]
    dirs = [x.reshape(B, -1, spec.num_dir_bins) for x in preds["dir"]]
    return spec, cls, box, dirs


# ------------------------------------------------------------------------------------------------ production size (on the GPU)
def pp_case(B=16, seed=0):
    from lidardetection_amd.pointpillar import PointPillarKITTI
    torch.manual_seed(seed)
    m = PointPillarKITTI.__new__(PointPillarKITTI)   # only what rpn_loss reads: no backbone, no voxeliser
    torch.nn.Module.__init__(m)
    m.nx, m.ny, m.num_class, m.pc_range = 432, 496, 3, [0.0, -39.68, -3.0, 69.12, 39.68, 1.0]
    m.anchors = torch.zeros(1, 7, device=DEV)
    head = m._loss_head()
    gt = random_gts(head.loss_anchors(), B, 60, seed)
    t = head.assign_targets(gt)
    N = t['box_cls_labels'].shape[1]
    g = torch.Generator(device="cpu").manual_seed(seed)
    cls = (torch.randn(B, 248, 216, 18, generator=g) * 2 - 2).to(DEV)
    box = (torch.randn(B, 248, 216, 42, generator=g) * 0.5).to(DEV)
    dirs = torch.randn(B, 248, 216, 12, generator=g).to(DEV)
    assert N == 321408
    return m, head, t, [cls], [box], [dirs], gt


def random_gts(anchors, B, M, seed):
    """(B, M, 8) KITTI gts on random anchors (jittered, so they match), of the anchor's class ([y, x, class, rot] order); frame 0
    has none, the others 0..M"""
    r = np.random.default_rng(seed)
    a = anchors.cpu().numpy()
    gt = np.zeros((B, M, 8), np.float32)
    for b in range(1, B):
        n = int(r.integers(0, M + 1))
        idx = r.integers(0, a.shape[0], n)
        gt[b, :n, :7] = a[idx, :7]
        gt[b, :n, :2] += r.uniform(-0.2, 0.2, (n, 2))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7] = 1 + (idx % 6) // 2
    return torch.from_numpy(gt).to(DEV)


def nus_case(B=4, seed=1):
    from lidardetection_amd.second_multihead import NUS_CLASSES, NUS_HEADS, SECONDMultiHeadNuScenes
    m = SECONDMultiHeadNuScenes.__new__(SECONDMultiHeadNuScenes)
    torch.nn.Module.__init__(m)
    m.grid, m.pc_range = [1024, 1024, 40], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    m.head_anchors = [torch.zeros(1, 7, device=DEV)]
    head = m._loss_head()
    anchors = head.loss_anchors()
    r = np.random.default_rng(seed)
    a = anchors.cpu().numpy()
    per_class = [int(np.prod(x.shape[:-1])) for x in head.anchors]
    starts = np.cumsum([0] + per_class)
    gt = np.zeros((B, 60, 10), np.float32)
    for b in range(B):
        n = int(r.integers(20, 61))
        cls_ids = r.integers(1, 11, n)
        idx = np.array([r.integers(starts[c - 1], starts[c]) for c in cls_ids])
        gt[b, :n, :7] = a[idx, :7]
        gt[b, :n, :2] += r.uniform(-0.2, 0.2, (n, 2))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7:9] = r.normal(0, 2, (n, 2))
        gt[b, :n:4, 7:9] = np.nan                               # NuScenes velocities that are missing
        gt[b, :n, 9] = cls_ids
    gt = torch.from_numpy(gt).to(DEV)
    t = head.assign_targets(gt)
    g = torch.Generator(device="cpu").manual_seed(seed)
    names = [c[0] for c in NUS_CLASSES]
    n_h = [sum(per_class[names.index(name)] for name in h) for h in NUS_HEADS]
    cls = [(torch.randn(B, n, len(h), generator=g) * 2 - 2).to(DEV) for n, h in zip(n_h, NUS_HEADS)]
    box = [(torch.randn(B, n, 10, generator=g) * 0.5).to(DEV) for n in n_h]
    return m, head, t, cls, box, gt
