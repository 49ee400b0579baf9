"""GPU checks of the fused train-mode PillarVFE and the differentiable PointPillarScatter (csrc/pfn_train.hip, pillar_ops.py):
against the reference's own train step (tests/golden/pfn_train_ref.npz), against the mirror's torch path in float64 at
PointPillar-KITTI bs 16, the mirror's dispatch, the scatter's backward in both memory formats, sync-freedom and bitwise
reproducibility, and PointPillarKITTI.train_loss end to end against the same model on the stock torch PFN and scatter."""
import os

import numpy as np
import pytest
import torch

from lidardetection_amd import pillar_ops, synth
from lidardetection_amd.pcdet.models.backbones_2d.map_to_bev.bev_maps import PointPillarScatter
from lidardetection_amd.pcdet.utils.cfg import AttrDict

from _gpu_util import no_host_sync, rel, release_memory  # noqa: F401  (release_memory: an autouse fixture)
from _pp_train_torch import DEV, bs16_voxels, pp_inputs, stock_loss, vfe

pytestmark = pytest.mark.gpu
CASES = ("kitti", "nus", "kitti_dist")


def _load(golden_dir, case):
    z = np.load(os.path.join(golden_dir, "pfn_train_ref.npz"))
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _canvas_grad(grad_pf, coords, B, C, nx, ny, channels_last, seed=0):
    """a canvas gradient that holds grad_pf at the pillars' cells and noise elsewhere (which the backward must ignore)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    G = torch.randn(B, C, ny, nx, generator=g).to(DEV)
    c = coords.long()
    G[c[:, 0], :, c[:, 2], c[:, 3]] = grad_pf
    return G.contiguous(memory_format=torch.channels_last) if channels_last else G.contiguous()


@pytest.mark.parametrize("case", CASES)
def test_kernels_match_reference_fixture(golden_dir, case):
    d = _load(golden_dir, case)
    vox, num, coords = _t(d["voxels"]), _t(d["num_points"]), _t(d["coords"])
    w = _t(d["weight"]).requires_grad_()
    gamma, beta = _t(d["gamma"]).requires_grad_(), _t(d["beta"]).requires_grad_()
    rm, rv = _t(d["rm0"]).clone(), _t(d["rv0"]).clone()
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    nx, ny = (int(v) for v in d["grid"])
    B = int(d["batch_size"])
    out, mean, var = pillar_ops.pillar_vfe_train(vox, num, coords, w, gamma, beta, rm, rv, d["voxel_size"], d["pc_range"],
                                                 with_distance=bool(d["with_distance"]), num_batches_tracked=nbt, return_stats=True)
    assert rel(out, _t(d["out64"])) < 1e-5
    torch.testing.assert_close(mean.double(), _t(d["mean64"]), rtol=1e-6, atol=1e-6 * float(np.abs(d["mean64"]).max()))
    torch.testing.assert_close(var.double(), _t(d["var64"]), rtol=1e-6, atol=0)
    torch.testing.assert_close(rm.double(), _t(d["rm1"]), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(rv.double(), _t(d["rv1"]), rtol=1e-6, atol=0)
    for channels_last in (False, True):
        for p in (w, gamma, beta):
            p.grad = None
        canvas = pillar_ops.pillar_scatter_train(out, coords, B, nx, ny, channels_last=channels_last)
        G = _canvas_grad(_t(d["grad_pf"]), coords, B, out.shape[1], nx, ny, channels_last)
        (canvas * G).sum().backward(retain_graph=True)
        for name, p in (("d_weight", w), ("d_gamma", gamma), ("d_beta", beta)):
            assert rel(p.grad, _t(d[name + "64"])) < 1e-5, (name, channels_last)
    pillar_ops.pillar_vfe_train(vox, num, coords, w, gamma, beta, rm, rv, d["voxel_size"], d["pc_range"],
                                with_distance=bool(d["with_distance"]), num_batches_tracked=nbt)
    torch.testing.assert_close(rm.double(), _t(d["rm2"]), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(rv.double(), _t(d["rv2"]), rtol=1e-6, atol=0)
    assert int(nbt) == int(d["nbt2"]) == 2


def test_production_size_against_the_torch_path_in_float64():
    vox, nv = bs16_voxels()
    assert nv > 100000
    total = vox["voxel_offsets"][16:17]
    m = vfe()
    layer = m.pfn_layers[0]
    ref = vfe()
    ref.double()
    g = torch.randn(vox["voxels"].shape[0], 64, device=DEV)
    out = pillar_ops.pillar_vfe_train(vox["voxels"], vox["voxel_num_points"], vox["voxel_coords"], layer.linear.weight, layer.norm.weight,
                                      layer.norm.bias, layer.norm.running_mean, layer.norm.running_var, synth.PP_VOXEL, synth.PP_RANGE,
                                      num_batches_tracked=layer.norm.num_batches_tracked, num_voxels_dev=total)
    (out * g).sum().backward()
    assert torch.isfinite(out).all() and (out[nv:] == 0).all()
    bd = ref({"voxels": vox["voxels"][:nv].double(), "voxel_num_points": vox["voxel_num_points"][:nv],
              "voxel_coords": vox["voxel_coords"][:nv]})
    want = bd["pillar_features"]
    (want * g[:nv].double()).sum().backward()
    assert rel(out[:nv], want) < 1e-5
    rl = ref.pfn_layers[0]
    torch.testing.assert_close(layer.norm.running_mean.double(), rl.norm.running_mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(layer.norm.running_var.double(), rl.norm.running_var, rtol=1e-6, atol=0)
    assert int(layer.norm.num_batches_tracked) == 1
    # fp32 rows against fp64 ones: a near-tie between two points of a pillar (or a ReLU edge) may select differently at this
    # size, moving one pillar's contribution; 1e-4 of the largest gradient leaves room for a few of them
    for a, b in ((layer.linear.weight, rl.linear.weight), (layer.norm.weight, rl.norm.weight), (layer.norm.bias, rl.norm.bias)):
        assert rel(a.grad, b.grad) < 1e-4


def test_mirror_dispatch(monkeypatch):
    vox, nv = bs16_voxels(B=2, seed=7)
    bd = lambda v: {"voxels": v, "voxel_num_points": vox["voxel_num_points"][:nv], "voxel_coords": vox["voxel_coords"][:nv]}  # noqa: E731
    calls = []
    train_fn, eval_fn = pillar_ops.pillar_vfe_train, pillar_ops.pillar_vfe
    monkeypatch.setattr(pillar_ops, "pillar_vfe_train", lambda *a, **k: calls.append("train") or train_fn(*a, **k))
    monkeypatch.setattr(pillar_ops, "pillar_vfe", lambda *a, **k: calls.append("eval") or eval_fn(*a, **k))
    m = vfe()
    v = vox["voxels"][:nv].contiguous()
    out = m(bd(v))["pillar_features"]
    assert calls == ["train"] and out.requires_grad
    m.eval()
    m(bd(v))
    assert calls == ["train", "eval"]
    m.train()
    vg = v.clone().requires_grad_()                  # gradients with respect to the voxels: the torch path
    m(bd(vg))["pillar_features"].sum().backward()
    assert calls == ["train", "eval"] and vg.grad is not None

    from lidardetection_amd.pointpillar import PointPillarKITTI
    pp = PointPillarKITTI(batch_size=2, device=DEV)
    before = [t.clone() for t in pp._pfn_folded()]
    pts, offs, gt = pp_inputs(2, 3)
    pp.train()
    sum(pp.train_loss(pts, offs, gt)).backward()
    pp.eval()
    w, s, t = pp._pfn_folded()
    n = pp.pfn_norm
    s_want, t_want = pillar_ops.fold_bn(n.weight.detach(), n.bias.detach(), n.running_mean, n.running_var, n.eps)
    assert not torch.equal(t, before[2]) and torch.equal(s, s_want) and torch.equal(t, t_want)
    assert int(n.num_batches_tracked) == 1


@pytest.mark.parametrize("channels_last", [False, True])
def test_scatter_autograd_matches_index_assign(channels_last):
    vox, nv = bs16_voxels(B=2, seed=3)
    coords = vox["voxel_coords"]
    total = vox["voxel_offsets"][2:3]
    V = coords.shape[0]
    feats = torch.randn(V, 64, device=DEV, requires_grad=True)
    canvas = pillar_ops.pillar_scatter_train(feats, coords, 2, 432, 496, num_voxels_dev=total, channels_last=channels_last)
    G = torch.randn(2, 64, 496, 432, device=DEV)
    G = G.contiguous(memory_format=torch.channels_last) if channels_last else G
    (canvas * G).sum().backward()
    f2 = feats.detach()[:nv].clone().requires_grad_()
    flat = torch.zeros(2, 64, 496 * 432, device=DEV)
    c = coords[:nv].long()
    flat[c[:, 0], :, c[:, 2] * 432 + c[:, 3]] = f2
    want = flat.view(2, 64, 496, 432)
    assert torch.equal(canvas, want)
    (want * G).sum().backward()
    assert torch.equal(feats.grad[:nv], f2.grad) and (feats.grad[nv:] == 0).all()
    # the mirror module takes the same path for grad-requiring features
    mod = PointPillarScatter(AttrDict(NUM_BEV_FEATURES=64), [432, 496, 1])
    f3 = feats.detach()[:nv].clone().requires_grad_()
    out = mod({"pillar_features": f3, "voxel_coords": coords[:nv], "batch_size": 2})["spatial_features"]
    assert out.grad_fn is not None and "PillarScatterTrain" in type(out.grad_fn).__name__
    (out * G).sum().backward()
    assert torch.equal(f3.grad, f2.grad)


def test_sync_free_and_bitwise_deterministic():
    vox, nv = bs16_voxels(seed=5)
    total = vox["voxel_offsets"][16:17]
    G = torch.randn(16, 64, 496, 432, device=DEV).contiguous(memory_format=torch.channels_last)
    runs = []
    torch.cuda.synchronize()
    for _ in range(2):
        m = vfe(seed=1)
        layer = m.pfn_layers[0]
        with no_host_sync():
            out = pillar_ops.pillar_vfe_train(vox["voxels"], vox["voxel_num_points"], vox["voxel_coords"], layer.linear.weight,
                                              layer.norm.weight, layer.norm.bias, layer.norm.running_mean, layer.norm.running_var,
                                              synth.PP_VOXEL, synth.PP_RANGE, num_batches_tracked=layer.norm.num_batches_tracked,
                                              num_voxels_dev=total)
            canvas = pillar_ops.pillar_scatter_train(out, vox["voxel_coords"], 16, 432, 496, num_voxels_dev=total, channels_last=True)
            (canvas * G).sum().backward()
        runs.append([out.detach().clone(), layer.norm.running_mean.clone(), layer.norm.running_var.clone(),
                     layer.linear.weight.grad.clone(), layer.norm.weight.grad.clone(), layer.norm.bias.grad.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


def test_train_loss_end_to_end_matches_stock_torch():
    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = pp_inputs(2, 11)
    models = []
    for _ in range(3):
        torch.manual_seed(4)
        models.append(PointPillarKITTI(batch_size=2, device=DEV).train())
    fused, stock, noisy = models
    with pytest.raises(pillar_ops._lib.LidarHipError):
        PointPillarKITTI(batch_size=2, device=DEV).train_loss(pts, offs, gt)      # eval mode: refused
    lf = fused.train_loss(pts, offs, gt)
    ls = stock_loss(stock, pts, offs, gt)
    for a, b in zip(lf, ls):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    sum(lf).backward()
    sum(ls).backward()
    # The stock step once more with its pillar features perturbed by fp32-rounding-sized noise (2^-24 relative): how far apart two
    # float32 backbones with train-mode BatchNorm put the gradients when their inputs differ only in the last bits.  (Their
    # convolution weight gradients are BatchNorm-normalised sums over the whole map: they cancel, and differ at ~1e-3 relative.)
    sum(stock_loss(noisy, pts, offs, gt, perturb=2.0 ** -24)).backward()
    named, noise = dict(stock.named_parameters()), dict(noisy.named_parameters())
    errs = {name: rel(p.grad, named[name].grad) for name, p in fused.named_parameters() if p.grad is not None}
    floor = {name: rel(noise[name].grad, named[name].grad) for name in named}
    assert len(errs) == len(named)
    bad = {k: (v, floor[k]) for k, v in errs.items() if not v < max(1e-4, 10 * floor[k])}
    assert not bad, bad
    torch.testing.assert_close(fused.pfn_norm.running_mean, stock.pfn_norm.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(fused.pfn_norm.running_var, stock.pfn_norm.running_var, rtol=1e-5, atol=1e-6)
    assert int(fused.pfn_norm.num_batches_tracked) == int(stock.pfn_norm.num_batches_tracked) == 1
