"""What tests/test_gpu_pfn_train.py, tools/pp_train_bench.py and tools/bev_train_bench.py share: the bs-16 PointPillar voxel
workload, the train-mode PillarVFE under test, the training inputs, and `stock_loss`, the same training step on the stock torch PFN
(the mirror's formulation) and torch index-assign scatter."""
import numpy as np
import torch
import torch.nn.functional as F

from lidardetection_amd import synth
from lidardetection_amd.pcdet.models.backbones_3d.vfe.encoders import PillarVFE
from lidardetection_amd.pcdet.utils.cfg import AttrDict
from lidardetection_amd.voxelizer import BatchVoxelizer

from _gpu_util import pp_inputs as _pp_inputs

DEV = torch.device("cuda:0")


def pp_cfg(**kw):
    return AttrDict(dict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[64], **kw))


def bs16_voxels(B=16, seed=0):
    frames = [synth.cloud_ring(2000 + seed + i) if i % 2 else synth.cloud_uniform(1000 + seed + i) for i in range(B)]
    pts = torch.from_numpy(np.concatenate(frames)).to(DEV)
    offs = torch.tensor(np.cumsum([0] + [len(f) for f in frames]), dtype=torch.int32, device=DEV)
    vz = BatchVoxelizer(synth.PP_VOXEL, synth.PP_RANGE, 32, 16000)
    vox = vz(pts, offs, max(len(f) for f in frames), compact=True)
    nv = int(vox["voxel_offsets"][B])
    for k, fill in (("voxels", float("nan")), ("voxel_coords", -7), ("voxel_num_points", -3)):
        vox[k][nv:] = fill                           # rows past the device count: neither read nor counted
    return vox, nv


def vfe(seed=0):
    torch.manual_seed(seed)
    m = PillarVFE(pp_cfg(), 4, synth.PP_VOXEL, synth.PP_RANGE).to(DEV)
    with torch.no_grad():
        bn = m.pfn_layers[0].norm
        bn.weight.uniform_(0.3, 1.5)
        bn.weight[::5] *= -1
        bn.bias.normal_(0, 0.3)
        bn.running_var.uniform_(0.8, 1.2)
    return m.train()


def pp_inputs(B, seed):
    return _pp_inputs(B, seed, 2100)


def stock_loss(m, pts, offs, gt, dt=torch.float64, perturb=0.0):
    """the same training step on the stock torch PFN (the mirror's formulation) and torch index-assign scatter.  The PFN runs in
    float64 (dt): in float32 its weight gradient sum(dz x) over ~10^6 rows cancels (sum dz = 0 under BatchNorm, |x| ~ 70 m) to a relative
    error of ~1e-3, which is the torch path's error, not the kernels' (they accumulate in fp64)."""
    with torch.no_grad():
        vox = m.voxelizer(pts, offs, m.n_max, compact=True)
    nv = int(vox["voxel_offsets"][m.B])
    v, num, coords = vox["voxels"][:nv].to(dt), vox["voxel_num_points"][:nv], vox["voxel_coords"][:nv]
    xyz = v[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / num.to(dt).view(-1, 1, 1)
    vs = torch.tensor(m.voxel_size, device=DEV, dtype=dt)
    centre = coords[:, [3, 2, 1]].to(dt) * vs + (vs / 2 + torch.tensor(m.pc_range[:3], device=DEV, dtype=dt))
    x = torch.cat([v, xyz - mean, xyz - centre.unsqueeze(1)], dim=-1)
    x = x * (torch.arange(v.shape[1], device=DEV).view(1, -1) < num.view(-1, 1)).unsqueeze(-1).to(dt)
    n = m.pfn_norm
    z = F.linear(x, m.pfn_linear.weight.to(dt))
    rm, rv = n.running_mean.to(dt, copy=True), n.running_var.to(dt, copy=True)
    y = F.batch_norm(z.transpose(1, 2), rm, rv, n.weight.to(dt), n.bias.to(dt), True, n.momentum, n.eps).transpose(1, 2)
    with torch.no_grad():
        n.running_mean.copy_(rm)
        n.running_var.copy_(rv)
        n.num_batches_tracked.add_(1)
    feat = torch.relu(y).amax(dim=1).float()
    if perturb:                                      # relative noise of the size of fp32 rounding (the test's noise floor)
        g = torch.Generator(device="cpu").manual_seed(1)
        feat = feat * (1 + perturb * torch.randn(feat.shape, generator=g)).to(DEV)
    flat = feat.new_zeros((m.B, 64, m.ny * m.nx))
    c = coords.long()
    flat[c[:, 0], :, c[:, 2] * m.nx + c[:, 3]] = feat
    canvas = flat.view(m.B, 64, m.ny, m.nx).contiguous(memory_format=torch.channels_last)
    return m.rpn_loss(m.backbone_head_stock(canvas), gt)
