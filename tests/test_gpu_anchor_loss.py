"""The fused anchor-head loss on the GPU (lidardetection_amd/anchor_loss.py, csrc/anchor_loss.hip) against the reference's own
get_loss (tests/golden/anchor_loss_ref.npz, written by tests/golden/make_loss_golden.py: fp32 and fp64 losses, fp64 autograd
gradients) and, at production size, against `restated_loss` (tests/test_anchor_loss_host.py), a torch restatement that must first
reproduce the fixture on the CPU.

Tolerances: losses 1e-5 relative; gradients 1e-5 x max |gradient| of their tensor, and exactly 0 where the reference's is."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from lidardetection_amd import anchor_loss
from lidardetection_amd.pcdet.utils.cfg import AttrDict

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_module():
    spec = importlib.util.spec_from_file_location("_anchor_loss_host_tests", os.path.join(HERE, "test_anchor_loss_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


H = _host_module()
DEV = torch.device("cuda:0")


def _fixture_inputs(name):
    meta, preds, grads, arr = H.load_case(name)
    spec = H.spec_of(meta)
    listed = meta["listed"]
    dev = lambda xs: [x.to(DEV).requires_grad_() for x in xs]   # noqa: E731
    p = {k: dev(v) for k, v in preds.items()}
    args = [p["cls"] if listed else p["cls"][0], p["box"] if listed else p["box"][0],
            (p["dir"] if listed else p["dir"][0]) if p["dir"] else None]
    return meta, spec, p, grads, arr, args


def _check_grads(leaves, grads, tol=1e-5):
    want = grads["cls"] + grads["box"] + grads["dir"]
    zero = grads["zero"]["cls"] + grads["zero"]["box"] + grads["zero"]["dir"]
    assert len(want) == len(leaves)
    for leaf, g, z in zip(leaves, want, zero):
        got = leaf.grad.double().cpu()
        g = g.double().reshape(got.shape)
        scale = g.abs().max().clamp(min=1e-30)
        err = ((got - g).abs() / scale).max().item()
        assert err < tol, err
        z = z.reshape(got.shape)
        assert (got[z] == 0).all(), "non-zero gradient where the reference's is exactly zero"


@pytest.mark.parametrize("name", H.CASES)
def test_fixture_losses_and_gradients(name):
    meta, spec, p, grads, arr, args = _fixture_inputs(name)
    labels = arr["labels"].to(DEV)
    losses = anchor_loss.anchor_head_loss(*args, labels, arr["targets"].to(DEV), arr["anchors"].to(DEV), spec)
    got = torch.stack([x.detach() for x in losses]).double().cpu()
    for ref in (arr["loss32"], arr["loss64"]):
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-12), (got, ref)
    sum(losses).backward()
    _check_grads(p["cls"] + p["box"] + p["dir"], grads)
    assert torch.equal(labels.cpu(), arr["labels"])   # the host op itself does not relabel


def _mirror(meta):
    from lidardetection_amd.pcdet.models.dense_heads.anchor_head_multi import AnchorHeadMulti
    from lidardetection_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
    cfg = AttrDict(meta["model_cfg"])
    cfg["LOSS_CONFIG"] = AttrDict(cfg["LOSS_CONFIG"])
    cfg["ANCHOR_GENERATOR_CONFIG"] = meta["anchor_generator_config"]
    coder = {"code_size": 9, "encode_angle_by_sincos": True} if meta["code_size"] == 10 else {}
    cfg["TARGET_ASSIGNER_CONFIG"] = AttrDict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                             NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder",
                                             BOX_CODER_CONFIG=coder)
    stride = meta["anchor_generator_config"][0]["feature_map_stride"]
    grid = np.array([meta["grid"][0] * stride, meta["grid"][1] * stride, 1])
    if meta["kind"] == "multi":
        cfg["RPN_HEAD_CFGS"] = [dict(HEAD_CLS_NAME=h) for h in meta["heads"]]
        return AnchorHeadMulti(cfg, 64, meta["num_class"], meta["class_names"], grid, meta["pc_range"], False)
    return AnchorHeadTemplate(cfg, meta["num_class"], meta["class_names"], grid, meta["pc_range"], False)


@pytest.mark.parametrize("name", H.CASES)
def test_mirror_get_loss(name):
    meta, spec, p, grads, arr, args = _fixture_inputs(name)
    with torch.cuda.device(DEV):
        head = _mirror(meta)
    assert head.loss_spec == spec
    assert torch.equal(head.loss_anchors().cpu(), arr["anchors"])     # the mirror's anchors are the reference's, in the loss order
    labels = arr["labels"].to(DEV)
    head.forward_ret_dict = dict(cls_preds=args[0], box_preds=args[1], box_cls_labels=labels,
                                 box_reg_targets=arr["targets"].to(DEV))
    if args[2] is not None:
        head.forward_ret_dict["dir_cls_preds"] = args[2]
    loss, tb = head.get_loss()
    assert set(tb) == set(meta["tb32"])
    for k, v in meta["tb32"].items():
        assert abs(tb[k] - v) <= 1e-5 * abs(v) + 1e-12, (k, tb[k], v)
    assert torch.equal(labels.cpu(), arr["labels_after"])             # num_class == 1: positives relabelled in place
    loss.backward()
    _check_grads(p["cls"] + p["box"] + p["dir"], grads)


def test_mirror_recomputes_for_new_or_modified_tensors():
    """the three loss methods share one fused call only while forward_ret_dict holds the same, unmodified tensors"""
    meta, spec, p, grads, arr, args = _fixture_inputs("kitti")
    with torch.cuda.device(DEV):
        head = _mirror(meta)
    targets = arr["targets"].to(DEV)

    def ret(cls):
        return dict(cls_preds=cls, box_preds=args[1], dir_cls_preds=args[2], box_cls_labels=arr["labels"].to(DEV),
                    box_reg_targets=targets)
    head.forward_ret_dict = ret(args[0])
    first, _ = head.get_cls_layer_loss()
    assert head.get_cls_layer_loss()[0] is first                       # same tensors: one fused call
    # a rebuilt dict with new tensors (the old ones freed first, so their ids may be reused) recomputes
    scaled = (args[0].detach() * 0.5).requires_grad_()
    del first
    head.forward_ret_dict = ret(scaled)
    got, _ = head.get_cls_layer_loss()
    ref = H.restated_loss([scaled.detach().reshape(meta["batch"], -1, 3)], [args[1].detach().reshape(meta["batch"], -1, 7)],
                          [args[2].detach().reshape(meta["batch"], -1, 2)], arr["labels"].to(DEV), targets, arr["anchors"].to(DEV),
                          spec)[0]
    assert abs(got.item() - ref.item()) <= 1e-5 * abs(ref.item())
    got.backward()
    assert scaled.grad is not None and scaled.grad.abs().max() > 0
    # an in-place change of a cached tensor recomputes too
    with torch.no_grad():
        scaled.mul_(2.0)
    again, _ = head.get_cls_layer_loss()
    assert again is not got and abs(again.item() - arr["loss32"][0].item()) <= 1e-5 * arr["loss32"][0].item()


# ------------------------------------------------------------------------------------------------ production size
def _pp_case(B=16, seed=0):
    from lidardetection_amd.pointpillar import PointPillarKITTI
    torch.manual_seed(seed)
    m = PointPillarKITTI.__new__(PointPillarKITTI)   # only what rpn_loss reads: no backbone, no voxeliser
    torch.nn.Module.__init__(m)
    m.nx, m.ny, m.num_class, m.pc_range = 432, 496, 3, [0.0, -39.68, -3.0, 69.12, 39.68, 1.0]
    m.anchors = torch.zeros(1, 7, device=DEV)
    head = m._loss_head()
    gt = _random_gts(head.loss_anchors(), B, 60, seed)
    t = head.assign_targets(gt)
    N = t['box_cls_labels'].shape[1]
    g = torch.Generator(device="cpu").manual_seed(seed)
    cls = (torch.randn(B, 248, 216, 18, generator=g) * 2 - 2).to(DEV)
    box = (torch.randn(B, 248, 216, 42, generator=g) * 0.5).to(DEV)
    dirs = torch.randn(B, 248, 216, 12, generator=g).to(DEV)
    assert N == 321408
    return m, head, t, [cls], [box], [dirs], gt


def _random_gts(anchors, B, M, seed):
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


def _check_against_restated(spec, cls, box, dirs, labels, targets, anchors, cols):
    B = labels.shape[0]
    nh = len(cls)
    leaves = [x.clone().requires_grad_() for x in cls + box + dirs]
    pick = lambda xs: xs if nh > 1 else xs[0]   # noqa: E731
    losses = anchor_loss.anchor_head_loss(pick(leaves[:nh]), pick(leaves[nh:2 * nh]), pick(leaves[2 * nh:]) if dirs else None,
                                          labels, targets, anchors, spec)
    sum(losses).backward()
    code = len(spec.code_weights)
    widths = cols + [code] * nh + [spec.num_dir_bins] * len(dirs)
    ref = [x.detach().double().reshape(B, -1, w).requires_grad_() for x, w in zip(cls + box + dirs, widths)]
    rl = H.restated_loss(ref[:nh], ref[nh:2 * nh], ref[2 * nh:], labels, targets, anchors, spec)
    sum(rl).backward()
    for a, b in zip(losses, rl):
        assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item()) + 1e-12, (a.item(), b.item())
    for leaf, r in zip(leaves, ref):
        g, rg = leaf.grad.double().reshape(r.shape), r.grad
        assert ((g - rg).abs().max() / rg.abs().max().clamp(min=1e-30)).item() < 1e-5
        assert (g[rg == 0] == 0).all()
    return losses, leaves


def test_production_pointpillar_kitti_bs16():
    m, head, t, cls, box, dirs, _ = _pp_case()
    labels, targets = t['box_cls_labels'], t['box_reg_targets']
    assert (labels > 0).sum().item() > 100 and (labels[0] > 0).sum().item() == 0
    _check_against_restated(head.loss_spec, cls, box, dirs, labels, targets, head.loss_anchors(), [3])


def _nus_case(B=4, seed=1):
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


def test_production_second_multihead_nuscenes_bs4():
    m, head, t, cls, box, _ = _nus_case()
    labels, targets = t['box_cls_labels'], t['box_reg_targets']
    assert torch.isnan(targets).any() and (labels > 0).sum().item() > 100
    _check_against_restated(head.loss_spec, cls, box, [], labels, targets, head.loss_anchors(), [c.shape[-1] for c in cls])


# ------------------------------------------------------------------------------------------------ end to end
def test_rpn_loss_hooks_train_the_stock_heads():
    from lidardetection_amd.pointpillar import PointPillarKITTI
    from lidardetection_amd.second_multihead import SECONDMultiHeadNuScenes
    torch.manual_seed(0)
    B = 2
    pp = PointPillarKITTI(batch_size=B, device=DEV, fold_bn=False).train()
    _, _, _, _, _, _, gt = _pp_case(B=B, seed=5)
    canvas = torch.randn(B, 64, pp.ny, pp.nx, device=DEV).contiguous(memory_format=torch.channels_last)
    sec = SECONDMultiHeadNuScenes(batch_size=B, device=DEV).train()
    _, _, _, _, _, ngt = _nus_case(B=B, seed=6)
    spatial = torch.randn(B, 512, 128, 128, device=DEV).contiguous(memory_format=torch.channels_last)
    for model, run, gts in [(pp, lambda: pp.backbone_head_stock(canvas), gt),
                            (sec, lambda: sec.heads_reference_layout(spatial), ngt)]:
        params = [p for p in model.parameters() if p.requires_grad]
        head_out = run()
        fused = model.rpn_loss(head_out, gts)
        g_fused = torch.autograd.grad(sum(fused), params, allow_unused=True)
        head_out = run()
        t = model._loss_head().assign_targets(gts)
        spec = model._loss_head().loss_spec
        if isinstance(head_out, list):
            cls, box, dirs = [c for c, _ in head_out], [b for _, b in head_out], []
        else:
            cls, box, dirs = [head_out[0]], [head_out[1]], [head_out[2]]
        ref = H.restated_loss(cls, box, dirs, t['box_cls_labels'], t['box_reg_targets'], model._loss_head().loss_anchors(), spec)
        for a, b in zip(fused, ref):
            assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item()) + 1e-12
        g_ref = torch.autograd.grad(sum(ref), params, allow_unused=True)
        n = 0
        for a, b in zip(g_fused, g_ref):
            if b is None:
                assert a is None or (a == 0).all()
                continue
            n += 1
            assert ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item() < 1e-4
        assert n > 0


def test_sync_free_and_bitwise_deterministic():
    m, head, _, cls, box, dirs, gt = _pp_case(B=16, seed=2)
    spec, anchors = head.loss_spec, head.loss_anchors()
    runs = []
    torch.cuda.synchronize()
    for _ in range(2):
        leaves = [x.clone().requires_grad_() for x in cls + box + dirs]
        torch.cuda.set_sync_debug_mode("error")
        try:
            t = head.assign_targets(gt)
            losses = anchor_loss.anchor_head_loss(leaves[0], leaves[1], leaves[2], t['box_cls_labels'], t['box_reg_targets'],
                                                  anchors, spec)
            sum(losses).backward()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        runs.append([x.detach().clone() for x in losses] + [x.grad.clone() for x in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))
