"""GPU checks of the PV-RCNN-KITTI training step: PVRCNNKitti.train_loss with sa="fused" against sa="stock" on
identical weights, inputs and random draws, two train_step iterations, and the argument checks."""
import numpy as np
import pytest
import torch

from _gpu_util import rel, release_memory  # noqa: F401  (release_memory: an autouse fixture)
from lidardetection_amd import _lib, optim, sa_train, synth
from lidardetection_amd.pvrcnn import PVRCNNKitti

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last
NOISE = 2.0 ** -17        # the noise floor of tests/test_gpu_second_train.py's fused-against-stock comparison
ROIS = 16


def _inputs(B, seed):
    """clouds of 4000 points per frame and 4 gt boxes in every frame but the last, which has none"""
    r = np.random.default_rng(seed)
    frames = []
    for i in range(B):
        c = synth.cloud_ring(2400 + seed + i)
        frames.append(c[np.sort(r.permutation(len(c))[:4000])])
    pts = torch.from_numpy(np.concatenate(frames)).to(DEV)
    sizes = [len(f) for f in frames]
    offs = torch.tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=DEV)
    gt = np.zeros((B, 6, 8), np.float32)
    size = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    for b in range(B - 1):
        n = 4
        cls = np.array([1, 2, 3, 1])
        gt[b, :n, 0], gt[b, :n, 1], gt[b, :n, 2] = r.uniform(5, 60, n), r.uniform(-30, 30, n), r.uniform(-1.5, -0.5, n)
        gt[b, :n, 3:6] = size[cls - 1] * r.uniform(0.9, 1.1, (n, 1))
        gt[b, :n, 6], gt[b, :n, 7] = r.uniform(-np.pi, np.pi, n), cls
    return pts, offs, sizes, torch.from_numpy(gt).to(DEV)


def _models(n, dropout_eval):
    models = []
    for _ in range(n):
        torch.manual_seed(6)
        m = PVRCNNKitti(batch_size=2, max_voxels=2000, num_keypoints=256, device=DEV).train()
        if dropout_eval:
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.eval()
        models.append(m)
    return models


def _draws(B, post=512):
    g = torch.Generator().manual_seed(12)
    return dict(fg_keys=torch.rand((B, post), generator=g).to(DEV), draws=torch.rand((B, ROIS), generator=g).to(DEV))


def test_pvrcnn_train_loss_fused_matches_stock(dev, monkeypatch):
    """the protocol of test_second_train_loss_fused_matches_stock: the five losses to rtol 1e-4, every parameter gradient within
    max(1e-4, 10 x the stock step's own spread under a 2^-17 relative perturbation of the BEV map) of the tensor's scale.  The fused
    route must have run in all six StackSAModuleMSG modules (two scales each) of the fused step and in none of the stock step.

    On random weights the RoI head's gradients (shared_fc_layer, cls_layers, reg_layers) spread by about 100 % of their scale under
    that perturbation, so this bound says little about them and about what reaches roi_grid_pool_layer through them; the gradients
    of a StackSAModuleMSG with the RoI-grid pool's widths are held to 1e-4 against the float64 replay in tests/test_gpu_sa_train.py."""
    pts, offs, sizes, gt = _inputs(2, 5)
    fused, stock, noisy = _models(3, dropout_eval=True)
    orig = noisy.backbone_head_stock
    canvas_noise = torch.Generator().manual_seed(9)
    seen = {}

    def perturbed(c):
        c2 = c * (1 + NOISE * torch.randn(c.shape, generator=canvas_noise).to(DEV).contiguous(memory_format=CL))
        seen["canvas"] = c2
        return orig(c2)
    noisy.backbone_head_stock = perturbed
    # the noisy model's second stage must read the perturbed map as well: train_trunk returns what backbone_head_stock was given
    trunk = noisy.train_trunk
    noisy.train_trunk = lambda *a, **k: (lambda h, ms, c: (h, ms, seen["canvas"]))(*trunk(*a, **k))
    kw = dict(target_config={"ROI_PER_IMAGE": ROIS}, **_draws(2))
    sa_modules = [fused.SA_rawpoints, *fused.SA_layers, fused.roi_grid_pool_layer]
    assert len(sa_modules) == 6 and all(sa_train.module_supported(m) for m in sa_modules)
    calls, orig_max = [], sa_train.bn_relu_max_forward
    monkeypatch.setattr(sa_train, "bn_relu_max_forward", lambda *a, **k: (calls.append(1), orig_max(*a, **k))[1])
    lf = fused.train_loss(pts, offs, sizes, gt, sa="fused", **kw)
    assert len(calls) == sum(len(m.mlps) for m in sa_modules) == 12, len(calls)
    ls = stock.train_loss(pts, offs, sizes, gt, sa="stock", **kw)
    ln = noisy.train_loss(pts, offs, sizes, gt, **kw)
    assert len(calls) == 12, "the stock step ran fused kernels"
    print("losses fused", [float(a.detach()) for a in lf], "stock", [float(a.detach()) for a in ls])
    assert len(lf) == len(ls) == 5
    for a, b in zip(lf, ls):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    for ll in (lf, ls, ln):
        sum(ll).backward()
    pf, ps, pn = dict(fused.named_parameters()), dict(stock.named_parameters()), dict(noisy.named_parameters())
    errs = {k: rel(p.grad, ps[k].grad, empty_ok=True) for k, p in pf.items() if p.grad is not None}
    assert len(errs) == len([k for k, p in ps.items() if p.grad is not None]) == len(ps)
    floors = {k: rel(pn[k].grad, ps[k].grad, empty_ok=True) for k in errs}
    worst = max(errs, key=lambda k: errs[k] / max(1e-4, 10 * floors[k]))
    print("worst", worst, f"{errs[worst]:.1e}", "floor", f"{floors[worst]:.1e}")
    for k in sorted(errs, key=lambda k: -errs[k])[:8]:
        print(f"  {k}: fused-stock {errs[k]:.1e} floor {floors[k]:.1e}")
    bad = {k: (v, floors[k]) for k, v in errs.items() if not v < max(1e-4, 10 * floors[k])}
    assert not bad, bad
    for (k, bf), bs in zip(fused.named_buffers(), stock.buffers()):
        if "running" in k:      # the gradients' criterion: the stock step's own spread under the perturbation is the floor
            assert rel(bf, bs, empty_ok=True) < max(1e-4, 10 * rel(dict(noisy.named_buffers())[k], bs, empty_ok=True)), k
        elif "num_batches" in k:
            assert int(bf) == int(bs) == 1


def test_pvrcnn_train_step_two_iterations(dev):
    pts, offs, sizes, gt = _inputs(2, 17)
    (model,) = _models(1, dropout_eval=False)
    # A randomly initialised RPN proposes no box near a hand-placed gt, and without a foreground RoI the box-regression branch has a
    # zero gradient.  So the first four proposals of every frame become its gt boxes: a first forward records the proposals (train-mode
    # BatchNorm normalises by batch statistics, so the steps below see the same ones).
    seen, orig = {}, model.rcnn_targets

    def record(rois, roi_scores, roi_labels, gt_boxes, **kw):
        seen["rois"], seen["labels"] = rois, roi_labels
        return orig(rois, roi_scores, roi_labels, gt_boxes, **kw)
    model.rcnn_targets = record
    model.train_loss(pts, offs, sizes, gt, target_config={"ROI_PER_IMAGE": ROIS})
    model.rcnn_targets = orig
    gt = torch.zeros_like(gt)
    gt[:, :4, :7], gt[:, :4, 7] = seen["rois"][:, :4], seen["labels"][:, :4].to(gt.dtype)
    assert bool((gt[:, :4, 3:6] > 0).all())
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    stats = {k: b.detach().clone() for k, b in model.named_buffers() if "running" in k}
    opt = optim.AdamOneCycle(model, wd=0.01, max_grad_norm=10.0)
    for it in range(2):
        opt.lr, opt.mom = optim.one_cycle(it, 10)
        out = model.train_step(pts, offs, sizes, gt, opt, sa="fused", sparse="fused", backbone="fused",
                               target_config={"ROI_PER_IMAGE": ROIS})
        assert len(out) == 6 and all(t.is_cuda and not t.requires_grad and bool(torch.isfinite(t).all()) for t in out)
        print("step", it, [float(t) for t in out])
    with_grad = [k for k, p in model.named_parameters() if p.grad is not None]
    assert len(with_grad) == len(before)
    still = [k for k in with_grad if torch.equal(dict(model.named_parameters())[k].detach(), before[k])]
    assert not still, still
    assert stats and all(not torch.equal(b, stats[k]) for k, b in model.named_buffers() if k in stats)


def test_pvrcnn_train_loss_argument_checks(dev):
    pts, offs, sizes, gt = _inputs(2, 5)
    (model,) = _models(1, dropout_eval=False)
    with pytest.raises(_lib.LidarHipError):
        model.train_loss(pts, offs, sizes, gt, sa="triton")
    model.eval()
    with pytest.raises(_lib.LidarHipError):
        model.train_loss(pts, offs, sizes, gt)
