"""CPU-only checks of the train-mode set abstraction: the float64 replay of tests/_sa_train_np.py against the
reference-form computation (the (M, C, nsample) grouping built from the same idx, then Conv2d / BatchNorm2d / ReLU / max_pool2d
modules in float64 under torch autograd), the argument validation of every csrc/sa_train.hip entry point (no device is touched),
the pure-host support predicates and workspace sizes, and the exclusion caps of the GPU tests on the reference alone."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _sa_train_np as ref
from lidardetection_amd import _lib, sa_train
from lidardetection_amd.pcdet.ops.pointnet2 import _common as pn_common

ERR_ARG = -1
WIDTH = 5


def _reference_form(xyz, feats, new_xyz, idx, xyz_cnt, new_cnt, mlp, grad_out):
    """StackSAModuleMSG.forward's stock body on the CPU in float64, the grouping indexed from `idx`"""
    M, ns = idx.shape
    N = xyz.shape[0]
    key = torch.from_numpy(ref.pair_keys(idx, xyz_cnt, new_cnt, N).reshape(M, ns))
    live = (key < N).unsqueeze(-1)
    safe = key.clamp(max=max(N - 1, 0))
    f = torch.from_numpy(feats).double().requires_grad_()
    x, q = torch.from_numpy(xyz).double(), torch.from_numpy(new_xyz).double()
    if N == 0:
        grouped = torch.zeros(M, ns, 3 + feats.shape[1], dtype=torch.float64)
    else:
        grouped = torch.cat((x[safe] - q[:, None, :], f[safe]), dim=-1) * live            # (M, ns, 3 + C); empty balls -> 0
    y = mlp(grouped.permute(2, 0, 1).unsqueeze(0))                                        # (1, C', M, ns)
    out = F.max_pool2d(y, kernel_size=[1, ns]).squeeze(-1)[0].t()                         # pointnet2_modules.py:84-90
    out.backward(torch.from_numpy(grad_out).double())
    return out.detach().numpy(), (f.grad.numpy() if f.grad is not None else np.zeros_like(feats, dtype=np.float64))


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30)) if want.size else 0.0


# every fixture with two layers (PV-RCNN's depth); three layers on the fixtures with more than one query (the 8 rows of fixture 1
# leave a third BatchNorm with channels of nearly no variance, where the two float64 computations agree to 1e-7 only)
REPLAY_CASES = [(c, 2) for c in ref.CASES] + [(c, 3) for c in ref.CASES if sum(c[2]) > 1]


@pytest.mark.parametrize("case,layers", REPLAY_CASES, ids=[f"seed{c[0]}-ns{c[3]}-H{c[4]}-L{n}" for c, n in REPLAY_CASES])
def test_replay_equals_reference_form(case, layers):
    seed, xyz_cnt, new_cnt, ns, H, radius = case
    xyz, feats, new_xyz = ref.cloud(seed, xyz_cnt, new_cnt, WIDTH)
    idx = ref.ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, ns)
    torch.manual_seed(seed)
    mlp = pn_common.shared_mlp([3 + WIDTH] + [H] * layers).double().train()
    with torch.no_grad():
        for k, p in mlp.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.rand_like(p) + (0.5 if k.endswith("weight") else -0.5))
                if k.endswith("weight"):
                    p[1::3] *= -1                                           # negative-gamma channels
    mods = list(mlp)
    M = idx.shape[0]
    grad_out = np.random.default_rng(seed + 7).standard_normal((M, H))
    want_out, want_df = _reference_form(xyz, feats, new_xyz, idx, xyz_cnt, new_cnt, mlp, grad_out)
    Ws = [c.weight.detach()[:, :, 0, 0].numpy() for c in mods[0::3]]
    Gs, Bs = [b.weight.detach().numpy() for b in mods[1::3]], [b.bias.detach().numpy() for b in mods[1::3]]
    kw = dict(weights=Ws, gammas=Gs, betas=Bs, eps=mods[1].eps, grad_out=grad_out)
    pre = ref.scale_replay(xyz, feats, new_xyz, idx, xyz_cnt, new_cnt, arg=np.zeros((M, H), np.uint8), **kw)["pre_last"]
    # the exclusion cap of the GPU tests, on the reference alone
    assert (np.abs(pre) < 1e-6).mean() <= 1e-3
    rep = ref.scale_replay(xyz, feats, new_xyz, idx, xyz_cnt, new_cnt, arg=ref.reference_arg(pre), **kw)
    errs = {"out": _rel(rep["out"], want_out), "d_feats": _rel(rep["d_feats"], want_df)}
    for j, (conv, bn) in enumerate(zip(mods[0::3], mods[1::3])):
        errs[f"dW{j}"] = _rel(rep["d_w"][j], conv.weight.grad[:, :, 0, 0].numpy())
        errs[f"dgamma{j}"] = _rel(rep["d_gamma"][j], bn.weight.grad.numpy())
        errs[f"dbeta{j}"] = _rel(rep["d_beta"][j], bn.bias.grad.numpy())
    print(errs)
    assert max(errs.values()) <= 1e-10, errs


def test_inverse_index_restatement():
    """row_start / pairs of the numpy restatement: every source's list ascending, duplicates kept, empty balls left out"""
    seed, xyz_cnt, new_cnt, ns, H, radius = ref.CASES[2]
    xyz, _, new_xyz = ref.cloud(seed, xyz_cnt, new_cnt, WIDTH)
    idx = ref.ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, ns)
    N = len(xyz)
    row_start, pairs = ref.inverse_index(idx, xyz_cnt, new_cnt, N)
    key = ref.pair_keys(idx, xyz_cnt, new_cnt, N)
    assert row_start[0] == 0 and row_start[N] == int((key < N).sum()) and len(pairs) == idx.size
    for n in range(N):
        lst = pairs[row_start[n]:row_start[n + 1]]
        assert (np.diff(lst) > 0).all() and (key[lst] == n).all()
    assert ((idx[:, 0] >= 0) & (idx[:, -1] == idx[:, 0])).any() and (idx[:, 0] < 0).any()       # padded and empty balls exist


def test_support_and_workspace_are_pure_host():
    L = _lib.lib()
    for H, ns, ok in [(4, 1, True), (128, 64, True), (64, 16, True), (0, 8, False), (132, 8, False), (6, 8, False), (16, 0, False),
                      (16, 65, False), (-4, 8, False)]:
        assert bool(L.lidar_sa_train_supported(H, ns)) == ok == sa_train.supported(H, ns), (H, ns)
    assert L.lidar_bn_relu_max_train_workspace_bytes(130, 16, 64) == L.lidar_bn_relu_train_workspace_bytes(130 * 16, 64) > 0
    assert L.lidar_bn_relu_max_train_workspace_bytes(130, 16, 6) == 0
    assert L.lidar_bn_relu_max_train_workspace_bytes(-1, 16, 64) == 0
    assert L.lidar_bn_relu_max_train_workspace_bytes(2 ** 27, 16, 64) == 0                    # M * nsample = 2^31
    mlp = pn_common.shared_mlp([8, 16, 16]).train()
    assert sa_train.scale_supported(mlp, 16) and not sa_train.scale_supported(mlp, 65)
    assert not sa_train.scale_supported(pn_common.shared_mlp([8, 16]).train(), 16)            # one layer only
    assert not sa_train.scale_supported(pn_common.shared_mlp([8, 6, 16]).train(), 16)         # a width outside the support
    assert not sa_train.scale_supported(pn_common.shared_mlp([8, 16, 16]).eval(), 16)
    odd = pn_common.shared_mlp([8, 16, 16]).train()
    odd[1] = nn.BatchNorm2d(16, momentum=None)
    assert not sa_train.scale_supported(odd, 16)
    assert not sa_train.fused_sa_train_enabled()
    with sa_train.fused_sa_train():
        assert sa_train.fused_sa_train_enabled()
        with sa_train.fused_sa_train(False):
            assert not sa_train.fused_sa_train_enabled()
    assert not sa_train.fused_sa_train_enabled()


def test_argument_validation_without_a_device():
    """every entry rejects arguments outside the declared support with LIDAR_ERR_ARG before any launch (0x1000 stands for an
    aligned device pointer that is never dereferenced; 0x1004 for a misaligned one)"""
    L = _lib.lib()
    p, bad = 0x1000, 0x1004
    gf = lambda B=2, M=10, N=50, H=16, ns=8, table=p, q=p, fc=p, idx=p, ic=p, z=p: L.lidar_sa_gather_train_forward(   # noqa: E731
        B, M, N, H, ns, table, q, fc, idx, ic, z, None)
    for kw in (dict(B=0), dict(M=-1), dict(N=-1), dict(H=0), dict(H=6), dict(H=132), dict(ns=0), dict(ns=65), dict(M=2 ** 27, ns=16),
               dict(table=None), dict(table=bad), dict(q=bad), dict(fc=None), dict(idx=None), dict(ic=None), dict(z=None), dict(z=bad)):
        assert gf(**kw) == ERR_ARG, kw
    assert gf(M=0, table=None, z=None) == 0                                                  # a zero size: no launch, success
    pk = lambda B=2, M=10, N=50, ns=8, fc=p, idx=p, ic=p, keys=p: L.lidar_sa_pair_keys(B, M, N, ns, fc, idx, ic, keys, None)   # noqa: E731
    for kw in (dict(B=0), dict(M=-1), dict(N=-1), dict(ns=0), dict(ns=65), dict(M=2 ** 27, ns=16), dict(fc=None), dict(idx=None),
               dict(ic=None), dict(keys=None)):
        assert pk(**kw) == ERR_ARG, kw
    assert pk(M=0, idx=None, keys=None) == 0
    for a in ((-1, 5, p, p), (2 ** 31, 5, p, p), (10, -1, p, p), (10, 5, None, p), (10, 5, p, None)):
        assert L.lidar_sa_row_start(*a, None) == ERR_ARG, a
    gb = lambda M=10, N=50, H=16, ns=8, dz=p, idx=p, rs=p, pairs=p, dt=p, dq=p: L.lidar_sa_gather_train_backward(   # noqa: E731
        M, N, H, ns, dz, idx, rs, pairs, dt, dq, None)
    for kw in (dict(M=-1), dict(N=-1), dict(H=2), dict(H=130), dict(H=256), dict(ns=0), dict(ns=128), dict(M=2 ** 27, ns=16),
               dict(dz=None), dict(dz=bad), dict(idx=None), dict(rs=None), dict(pairs=None), dict(dt=None), dict(dt=bad), dict(dq=bad)):
        assert gb(**kw) == ERR_ARG, kw
    assert gb(M=0, N=0, dz=None, idx=None, rs=None, pairs=None, dt=None, dq=None) == 0
    ws = 1 << 20
    mf = lambda z=p, M=10, ns=8, H=16, g=p, b=p, eps=1e-5, out=p, arg=p, st=p, ss=p, bs=p, w=p, wb=ws: (   # noqa: E731
        L.lidar_bn_relu_max_train_forward(z, M, ns, H, g, b, eps, out, arg, st, ss, bs, w, wb, None))
    for kw in (dict(z=None), dict(z=bad), dict(M=-1), dict(M=0), dict(M=1, ns=1), dict(ns=0), dict(ns=65), dict(H=6), dict(H=132),
               dict(M=2 ** 27, ns=16), dict(g=None), dict(b=None), dict(eps=-1.0), dict(out=None), dict(out=bad), dict(arg=None),
               dict(st=None), dict(ss=None), dict(bs=None), dict(w=None)):
        assert mf(**kw) == ERR_ARG, kw
    assert mf(wb=16) == -3                                                                    # LIDAR_ERR_WORKSPACE
    mb = lambda z=p, M=10, ns=8, H=16, go=p, arg=p, g=p, st=p, ss=p, dz=p, dg=p, db=p, w=p, wb=ws: (   # noqa: E731
        L.lidar_bn_relu_max_train_backward(z, M, ns, H, go, arg, g, st, ss, dz, dg, db, w, wb, None))
    for kw in (dict(z=None), dict(M=-1), dict(M=1, ns=1), dict(ns=0), dict(ns=65), dict(H=6), dict(H=132), dict(M=2 ** 27, ns=16),
               dict(go=None), dict(go=bad), dict(arg=None), dict(g=None), dict(st=None), dict(ss=None), dict(dz=None), dict(dz=bad),
               dict(dg=None), dict(db=None), dict(w=None)):
        assert mb(**kw) == ERR_ARG, kw
    assert mb(wb=16) == -3


def test_wrappers_refuse_cpu_tensors():
    z = torch.zeros(16, 8)
    with pytest.raises(_lib.LidarHipError):
        sa_train.bn_relu_max_forward(z, 2, 8, torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(_lib.LidarHipError):
        sa_train.sa_gather_forward(torch.zeros(4, 8), None, torch.zeros(2, 8, dtype=torch.int32), torch.tensor([4], dtype=torch.int32),
                                   torch.tensor([2], dtype=torch.int32))
