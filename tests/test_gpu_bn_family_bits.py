"""Bit-for-bit pins of the fused train-mode BatchNorm family beside the plain segment path (which tests/test_gpu_second_train.py pins
with tests/golden/bn_relu_train_parent.npz): the residual rows form (lidar_bn_add_relu_train_*), the BatchNorm + ReLU + max form
(lidar_bn_relu_max_train_*) and PillarVFE's train step (lidar_pfn_train_*, whose partial sums go through the shared ordered reduce).
Every tests/golden/bn_family_*.npz holds this repository's own output on an MI355X from before the shared element math, launch
helpers and reduce kernel were factored out, with the input it was computed from."""
import os

import numpy as np
import pytest
import torch

from lidardetection_amd import pillar_ops, sa_train
from lidardetection_amd.spconv import train as rows_train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-3

# (N, C): Q = 16, R = 16 and one block (the 4-in-flight and 2-in-flight main loops and both tails) | Q = 6, R = 42 (four dead lanes,
# N barely above R)
ROWS_CASES = [(150, 64), (45, 24)]
# (M, nsample, H); the second has 320 rows: two blocks of partials
MAX_CASES = [(37, 5, 24), (20, 16, 64)]
PFN_CASE = dict(V=70, P=20, C=4, cout=64, count=66)       # three blocks of partials, four rows past the device count
PFN_VOXEL, PFN_RANGE = [0.16, 0.16, 4.0], [0.0, -39.68, -3.0, 69.12, 39.68, 1.0]


def _t(a):
    return torch.from_numpy(a).to(DEV)


def _np(d):
    return {k: v.detach().contiguous().cpu().numpy() for k, v in d.items()}


def rows_inputs(N, C):
    r = np.random.default_rng(1000 * N + C)
    f = lambda *s: r.standard_normal(s).astype(np.float32)          # noqa: E731
    return dict(z=f(N, C) * np.float32(1.3) + np.float32(0.2), r=f(N, C), G=f(N, C), gamma=r.uniform(0.5, 1.5, C).astype(np.float32),
                beta=r.uniform(-0.3, 0.3, C).astype(np.float32))


def run_rows(inp):
    """spconv.train.bn_relu_rows_forward / _backward with a residual (lidar_bn_add_relu_train_*)"""
    z, r, G, gamma, beta = (_t(inp[k]) for k in ("z", "r", "G", "gamma", "beta"))
    y, stats, scale_shift, batch_stats = rows_train.bn_relu_rows_forward(z, gamma, beta, EPS, residual=r)
    dz, d_r, d_gamma, d_beta = rows_train.bn_relu_rows_backward(z, G, gamma, stats, scale_shift, residual=r)
    return _np(dict(y=y, stats=stats, scale_shift=scale_shift, batch_stats=batch_stats, dz=dz, d_r=d_r, d_gamma=d_gamma, d_beta=d_beta))


def max_inputs(M, ns, H):
    r = np.random.default_rng(100000 * M + 1000 * ns + H)
    z = r.standard_normal((M, ns, H)).astype(np.float32)
    z[[0, M // 2, M - 1]] = 0.0                    # empty balls: every row exactly zero, equal maxima, arg must be the lowest s
    gamma = r.uniform(0.5, 1.5, H).astype(np.float32)
    gamma[::3] *= -1.0                             # a third of the channels take the minimum of z
    return dict(z=z.reshape(M * ns, H), G=r.standard_normal((M, H)).astype(np.float32), gamma=gamma,
                beta=r.uniform(-0.3, 0.3, H).astype(np.float32))


def run_max(inp, M, ns):
    """sa_train.bn_relu_max_forward / _backward (lidar_bn_relu_max_train_*)"""
    z, G, gamma, beta = (_t(inp[k]) for k in ("z", "G", "gamma", "beta"))
    out, arg, stats, scale_shift, batch_stats = sa_train.bn_relu_max_forward(z, M, ns, gamma, beta, EPS)
    dz, d_gamma, d_beta = sa_train.bn_relu_max_backward(z, M, ns, G, arg, gamma, stats, scale_shift)
    return _np(dict(out=out, arg=arg, stats=stats, scale_shift=scale_shift, batch_stats=batch_stats, dz=dz, d_gamma=d_gamma,
                    d_beta=d_beta))


def pfn_inputs():
    V, P, C, cout = (PFN_CASE[k] for k in ("V", "P", "C", "cout"))
    r = np.random.default_rng(70204)
    num = r.integers(2, P, V).astype(np.int32)
    num[::9] = P                                   # full pillars
    num[4::9] = 1                                  # a single point: the padded row's z = 0 competes in every channel
    coords = np.stack([r.integers(0, 2, V), np.zeros(V, np.int64), r.integers(0, 496, V), r.integers(0, 432, V)], 1).astype(np.int32)
    centre = np.stack([coords[:, 3] * 0.16 + 0.08, coords[:, 2] * 0.16 + 0.08 - 39.68], 1).astype(np.float32)
    vox = np.zeros((V, P, C), np.float32)
    vox[:, :, :2] = centre[:, None, :] + r.uniform(-0.08, 0.08, (V, P, 2)).astype(np.float32)
    vox[:, :, 2] = r.uniform(-3.0, 1.0, (V, P)).astype(np.float32)
    vox[:, :, 3] = r.uniform(0.0, 1.0, (V, P)).astype(np.float32)
    vox[np.arange(P)[None, :] >= num[:, None]] = 0.0
    gamma = r.uniform(0.3, 1.5, cout).astype(np.float32)
    gamma[::7] *= -1.0
    return dict(voxels=vox, num_points=num, coords=coords, weight=(r.standard_normal((cout, C + 6)) * 0.3).astype(np.float32),
                gamma=gamma, beta=(r.standard_normal(cout) * 0.3).astype(np.float32),
                rm0=(r.standard_normal(cout) * 0.1).astype(np.float32), rv0=r.uniform(0.8, 1.2, cout).astype(np.float32),
                G=r.standard_normal((V, cout)).astype(np.float32))


def run_pfn(inp):
    """pillar_ops.pillar_vfe_train (lidar_pfn_train_*) with a device voxel count below V, and its backward for a fixed upstream gradient"""
    w, gamma, beta = (_t(inp[k]).requires_grad_() for k in ("weight", "gamma", "beta"))
    rm, rv = _t(inp["rm0"]).clone(), _t(inp["rv0"]).clone()
    count = torch.tensor([PFN_CASE["count"]], dtype=torch.int32, device=DEV)
    out = pillar_ops.pillar_vfe_train(_t(inp["voxels"]), _t(inp["num_points"]), _t(inp["coords"]), w, gamma, beta, rm, rv, PFN_VOXEL,
                                      PFN_RANGE, num_voxels_dev=count)
    out.backward(_t(inp["G"]))
    return _np(dict(out=out, running_mean=rm, running_var=rv, d_weight=w.grad, d_gamma=gamma.grad, d_beta=beta.grad))


def _check(name, inp, out, outputs):
    gold = np.load(os.path.join(GOLDEN, name))
    for k, v in inp.items():
        assert np.array_equal(gold["in_" + k], v), k                  # the generator still produces the recorded input
    assert sorted(out) == sorted(outputs)
    for k, v in out.items():
        assert v.dtype == gold[k].dtype and v.shape == gold[k].shape, k
        assert np.array_equal(v.reshape(-1).view(np.uint8), gold[k].reshape(-1).view(np.uint8)), k


@pytest.mark.parametrize("N,C", ROWS_CASES)
def test_residual_rows_keep_their_bits(dev, N, C):
    inp = rows_inputs(N, C)
    _check(f"bn_family_rows_{N}x{C}.npz", inp, run_rows(inp), ("y", "stats", "scale_shift", "batch_stats", "dz", "d_r", "d_gamma", "d_beta"))


@pytest.mark.parametrize("M,ns,H", MAX_CASES)
def test_max_form_keeps_its_bits(dev, M, ns, H):
    inp = max_inputs(M, ns, H)
    out = run_max(inp, M, ns)
    empty = out["arg"][[0, M // 2, M - 1]]
    assert (empty == 0).all()                                         # equal maxima: the lowest s
    _check(f"bn_family_max_{M}x{ns}x{H}.npz", inp, out, ("out", "arg", "stats", "scale_shift", "batch_stats", "dz", "d_gamma", "d_beta"))


def test_pillar_vfe_train_keeps_its_bits(dev):
    inp = pfn_inputs()
    out = run_pfn(inp)
    assert not out["out"][PFN_CASE["count"]:].any()                   # rows past the device count are zero
    _check("bn_family_pfn.npz", inp, out, ("out", "running_mean", "running_var", "d_weight", "d_gamma", "d_beta"))
