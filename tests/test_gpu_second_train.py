"""GPU checks of the SECOND-KITTI training step: the differentiable HeightCompression (csrc/sparse_train.hip) bit for
bit against the stock index_put path, the fused train-mode BatchNorm1d + ReLU on sparse features and its residual form
(csrc/bn_train.hip) against float64 torch on the CPU, both sparse backbones under spconv.fused_bn_train against the fp64 replay
(oracle/spconv_grad_oracle.py), SECONDKitti.train_loss fused against stock, and two train_step iterations."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gpu_util import rel, release_memory  # noqa: F401  (release_memory: an autouse fixture)
from lidardetection_amd import bev_train, spconv, synth
from lidardetection_amd.pcdet.models.backbones_3d import spconv_backbone
from lidardetection_amd.pcdet.utils.cfg import AttrDict
from lidardetection_amd.spconv import tensor as sp_tensor
from lidardetection_amd.voxelizer import BatchVoxelizer, grid_size_of
from oracle import spconv_grad_oracle as go, spconv_sparse_oracle as sp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_relu_train_parent.npz")


# ---- 1. HeightCompression: forward and gradient bit for bit against the stock path ---------------------------------------------
def _sites(B, D, H, W, pattern, seed):
    """unique random [b, z, y, x] rows in a shuffled order; "empty_frame": frame 0 holds none; "n0": no row at all"""
    if pattern == "n0":
        return np.zeros((0, 4), np.int32)
    r = np.random.default_rng(seed)
    per = D * H * W
    frames = [1] if pattern == "empty_frame" else list(range(B))
    rows = []
    for b in frames:
        flat = r.choice(per, min(24, (2 * per) // 3), replace=False)
        z, rem = np.divmod(flat, H * W)
        y, x = np.divmod(rem, W)
        rows.append(np.stack([np.full_like(z, b), z, y, x], 1))
    idx = np.concatenate(rows)
    return idx[r.permutation(idx.shape[0])].astype(np.int32)


def _bev_pair(idx, C, B, D, H, W, seed):
    """(new dense_bev output, its features), (the old expression's output, its features) on clones of one feature matrix"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(idx.shape[0], C, generator=g).to(DEV)
    ind = torch.from_numpy(idx).to(DEV)
    f1, f2 = f.clone().requires_grad_(True), f.clone().requires_grad_(True)
    new = spconv.SparseConvTensor(f1, ind, [D, H, W], B).dense_bev()
    old = spconv.SparseConvTensor(f2, ind, [D, H, W], B).dense().view(B, C * D, H, W).contiguous(memory_format=CL)
    return (new, f1), (old, f2)


@pytest.mark.parametrize("pattern", ["random", "empty_frame", "n0"])
@pytest.mark.parametrize("C", [4, 8, 128])
@pytest.mark.parametrize("D,H,W", [(1, 3, 5), (2, 5, 7), (3, 4, 4), (4, 2, 9)])
def test_dense_bev_forward_and_gradient_equal_the_stock_path_bitwise(dev, D, H, W, C, pattern):
    B = 2
    idx = _sites(B, D, H, W, pattern, 100 * D + C)
    (new, f1), (old, f2) = _bev_pair(idx, C, B, D, H, W, 7 * D + C)
    if idx.shape[0]:
        assert "_DenseBEV" in type(new.grad_fn).__name__             # the kernel path, not the fallback
    assert new.shape == old.shape and new.stride() == old.stride() and torch.equal(new, old)
    G = torch.randn(B, C * D, H, W, generator=torch.Generator().manual_seed(3)).to(DEV).contiguous(memory_format=CL)
    junk = torch.full((max(idx.shape[0], 1), C), float("nan"), device=DEV)     # freed: a row nobody writes is not a lucky zero
    del junk
    new.backward(G)
    old.backward(G)
    assert f1.grad.shape == f2.grad.shape and torch.equal(f1.grad, f2.grad)
    # without a gradient the forward stays the one-pass kernel and the same bits
    with torch.no_grad():
        plain = spconv.SparseConvTensor(f1.detach(), torch.from_numpy(idx).to(DEV), [D, H, W], B).dense_bev() if idx.shape[0] else old
    assert torch.equal(plain, old)


@pytest.mark.parametrize("off", [8, 6])
def test_dense_bev_gradient_as_a_channel_slice_of_a_wider_map(dev, off):
    """g_ld > C * D and a non-zero channel offset; off = 8 takes the 16-byte loads, off = 6 the scalar ones"""
    B, D, H, W, C = 2, 2, 5, 7, 8
    idx = _sites(B, D, H, W, "random", 5)
    (new, f1), (old, f2) = _bev_pair(idx, C, B, D, H, W, 6)
    wide = torch.randn(B, C * D + 24, H, W, generator=torch.Generator().manual_seed(4)).to(DEV).contiguous(memory_format=CL)
    g = wide[:, off:off + C * D]
    assert g.stride(3) == C * D + 24 and not g.is_contiguous(memory_format=CL)
    old.backward(g)
    new.backward(g)                                                  # the slice itself reaches the kernel (pointer at the slice)
    assert torch.equal(f1.grad, f2.grad)
    direct = sp_tensor.dense_bev_backward(wide, torch.from_numpy(idx).to(DEV), C, D, offset=off)      # base pointer + g_off
    assert torch.equal(direct, f2.grad)


def test_dense_bev_gradient_of_rows_outside_the_volume_is_exactly_zero(dev):
    """the forward's scatter_index_kernel skips b outside [0, B) and z / y / x outside the volume: those rows get a zero gradient"""
    B, D, H, W, C = 2, 3, 4, 5, 8
    idx = _sites(B, D, H, W, "random", 9)
    bad = np.array([[B, 0, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, D, 0, 0], [1, 0, H, 0], [1, 0, -1, 0], [0, 1, 1, W], [0, 1, 1, -1],
                    [0, D - 1, H, 0], [1, -1, H, 0]], np.int32)
    allidx = np.concatenate([idx[:10], bad, idx[10:]])
    G = torch.randn(B, C * D, H, W, generator=torch.Generator().manual_seed(2)).to(DEV).contiguous(memory_format=CL)
    got = sp_tensor.dense_bev_backward(G, torch.from_numpy(allidx).to(DEV), C, D).cpu()
    Gc = G.cpu().view(B, C, D, H, W)
    want = torch.zeros(allidx.shape[0], C)
    for i, (b, z, y, x) in enumerate(allidx.tolist()):
        if 0 <= b < B and 0 <= z < D and 0 <= y < H and 0 <= x < W:
            want[i] = Gc[b, :, z, y, x]
    assert torch.equal(got, want) and bool((got[10:20] == 0).all())
    empty = sp_tensor.dense_bev_backward(G, torch.zeros((0, 4), dtype=torch.int32, device=DEV), C, D)
    assert empty.shape == (0, C)


# ---- 2. fused train-mode BatchNorm1d + ReLU on (N, C) features, plain and residual ----------------------------------------------
EPS, MOM = 1e-3, 0.01


def _bn_case(N, C, residual, seed):
    """inputs of one case on the CPU (fp32): z with channel 1 constant (variance 0) and channel 2 driven all-negative by its
    beta (and residual), gamma, beta, the residual, the upstream gradient and fresh running statistics"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, generator=g) * torch.linspace(0.5, 2.0, C) + torch.linspace(-1.0, 1.0, C)
    z[:, 1] = 0.7
    gamma = torch.empty(C).uniform_(0.5, 1.5, generator=g)
    beta = torch.empty(C).uniform_(-0.3, 0.3, generator=g)
    beta[1], beta[2] = 0.25, -100.0
    r = None
    if residual:
        r = torch.randn(N, C, generator=g)
        r[:, 2] = -r[:, 2].abs()
    G = torch.randn(N, C, generator=g)
    rm, rv = torch.empty(C).uniform_(-0.1, 0.1, generator=g), torch.empty(C).uniform_(0.8, 1.2, generator=g)
    return z, gamma, beta, r, G, rm, rv


def _bn_reference(z, gamma, beta, r, G, rm, rv):
    """float64 torch on the CPU -> (pre-activation, y, dz, d_r, d_gamma, d_beta, running mean, running variance)"""
    z64, g64, b64 = (t.double().requires_grad_(True) for t in (z, gamma, beta))
    r64 = r.double().requires_grad_(True) if r is not None else None
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    pre = F.batch_norm(z64, rm64, rv64, g64, b64, True, MOM, EPS)
    if r64 is not None:
        pre = pre + r64
    y = torch.relu(pre)
    y.backward(G.double())
    return pre.detach(), y.detach(), z64.grad, None if r64 is None else r64.grad, g64.grad, b64.grad, rm64, rv64


def _bn_gpu(z, gamma, beta, r, G, rm, rv):
    bn = torch.nn.BatchNorm1d(z.shape[1], eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    bn = bn.to(DEV).train()
    zd = z.to(DEV).requires_grad_(True)
    rd = r.to(DEV).requires_grad_(True) if r is not None else None
    y = spconv.bn_relu_train(zd, bn, rd)
    y.backward(G.to(DEV))
    assert int(bn.num_batches_tracked) == 1
    return y.detach(), zd.grad, None if rd is None else rd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [16, 32, 64, 128])
@pytest.mark.parametrize("N", [2, 3, 257, 5000])
def test_sparse_bn_relu_train_against_float64(dev, N, C, residual):
    """y, dz, d_r, d_gamma, d_beta and the updated running statistics against F.batch_norm (+ add) + relu in float64 on the CPU, each
    within 1e-4 of the tensor's max |ref|.  Elements whose fp64 pre-activation lies within 1e-6 of zero are excluded from the
    gradients by zeroing their upstream gradient in both runs (an fp32 ReLU gate may fall on either side there); the seeds leave
    at most 0.1 % of the elements there (asserted, on the CPU, before anything runs on the device).  Two runs are bitwise equal."""
    z, gamma, beta, r, G, rm, rv = _bn_case(N, C, residual, 1000 * N + C + int(residual))
    pre = _bn_reference(z, gamma, beta, r, G, rm, rv)[0]
    near = pre.abs() < 1e-6
    assert int(near.sum()) <= 1e-3 * near.numel(), int(near.sum())
    G = G.masked_fill(near, 0.0)
    ref = _bn_reference(z, gamma, beta, r, G, rm, rv)[1:]
    assert bool((ref[0][:, 2] == 0).all()) and bool((z[:, 1] == z[0, 1]).all())     # the all-negative and the constant channel
    got = _bn_gpu(z, gamma, beta, r, G, rm, rv)
    again = _bn_gpu(z, gamma, beta, r, G, rm, rv)
    errs = {}
    for name, a, b, w in zip(("y", "dz", "d_r", "d_gamma", "d_beta", "running_mean", "running_var"), got, again, ref):
        if w is None:
            assert a is None
            continue
        assert torch.equal(a, b), f"{name}: two runs differ"
        errs[name] = rel(a, w, empty_ok=True)
    print("bn", (N, C, residual), {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v <= 1e-4 for v in errs.values()), errs


def _parent_case_inputs():
    """the fixed input of the golden: two segments (a 32-channel slice of a 48-channel map, and a 16-channel map), 2 x 9 x 7 pixels"""
    r = np.random.default_rng(20)
    wide = (r.standard_normal((2, 9, 7, 48)) * 1.3 + 0.2).astype(np.float32)
    z2 = r.standard_normal((2, 9, 7, 16)).astype(np.float32)
    gamma, beta = r.uniform(0.5, 1.5, 48).astype(np.float32), r.uniform(-0.3, 0.3, 48).astype(np.float32)
    G = r.standard_normal((2, 9, 7, 48)).astype(np.float32)
    return dict(wide=wide, z2=z2, gamma=gamma, beta=beta, G=G)


def _run_parent_case(inp):
    """bev_train.bn_relu_forward / bn_relu_backward (lidar_bn_relu_train_*) on the golden's input -> its outputs as numpy arrays"""
    nhwc = lambda a: torch.from_numpy(a).to(DEV).permute(0, 3, 1, 2)            # noqa: E731  (B, C, H, W) with channels-last strides
    wide, z2, G = nhwc(inp["wide"]), nhwc(inp["z2"]), nhwc(inp["G"])
    zs = [wide[:, 8:40], z2]
    gamma, beta = torch.from_numpy(inp["gamma"]).to(DEV), torch.from_numpy(inp["beta"]).to(DEV)
    y, stats, scale_shift, batch_stats = bev_train.bn_relu_forward(zs, gamma, beta, 1e-3)
    dzs, d_gamma, d_beta = bev_train.bn_relu_backward(zs, G, gamma, stats, scale_shift)
    out = dict(y=y.permute(0, 2, 3, 1), stats=stats, scale_shift=scale_shift, batch_stats=batch_stats, dz0=dzs[0].permute(0, 2, 3, 1),
               dz1=dzs[1].permute(0, 2, 3, 1), d_gamma=d_gamma, d_beta=d_beta)
    return {k: v.contiguous().cpu().numpy() for k, v in out.items()}


def test_existing_bn_relu_train_entry_points_keep_their_bits(dev):
    """tests/golden/bn_relu_train_parent.npz: what lidar_bn_relu_train_forward / _backward gave on this input before the residual
    form was templated into their kernels (this repository's own output on an MI355X).  Every output equal bit for bit."""
    gold = np.load(GOLDEN)
    inp = _parent_case_inputs()
    for k, v in inp.items():
        assert np.array_equal(gold["in_" + k], v), k                  # the generator still produces the recorded input
    out = _run_parent_case(inp)
    for k, v in out.items():
        assert v.dtype == gold[k].dtype and np.array_equal(v.view(np.uint8), gold[k].view(np.uint8)), k


# ---- 3. both sparse backbones under spconv.fused_bn_train against the fp64 replay ------------------------------------------------
DATA = {"kitti": (synth.SEC_VOXEL, synth.SEC_RANGE, 5, 16000, 4), "nus": (synth.NUS_VOXEL, synth.NUS_RANGE, 10, 60000, 5)}


def _voxels(data, n_frames):
    vs, rng, pmax, vmax, C = DATA[data]
    frames = [synth.cloud_ring(2000 + f) if data == "kitti" else synth.cloud_nus(4000 + f) for f in range(n_frames)]
    out = BatchVoxelizer(vs, rng, pmax, vmax, C).voxelize_frames(frames, device=DEV)
    n = out["voxel_num_points"].clamp(min=1).float()
    feats = out["voxels"].sum(1) / n[:, None]
    zyx = [int(v) for v in grid_size_of(vs, rng)][::-1]
    return feats, out["voxel_coords"].int(), [zyx[0] + 1, zyx[1], zyx[2]]


def _site_weights(idx, C):
    """fixed loss weight per (site, channel), a function of (b, z, y, x) only: GPU and replay agree without matching row orders"""
    i = np.asarray(idx, np.float64)
    ph = 0.9 * i[:, :1] + 0.37 * i[:, 1:2] + 0.013 * i[:, 2:3] + 0.011 * i[:, 3:4]
    return np.cos(ph + 0.21 * np.arange(C)[None, :])


def _scaled_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    return err / max(scale, 1e-30)


_CROPS = {}


def _cropped(data):
    """the cropped two-frame input of test_gpu_spconv_train.test_backbone_train_step_matches_fp64_replay: 3000 + 12 voxels"""
    if data not in _CROPS:
        feats, coords, shape = _voxels(data, 2)
        idx = coords.cpu().numpy().astype(np.int64)
        keep = []
        for b, n in ((0, 3000), (1, 12)):
            rows = np.nonzero(idx[:, 0] == b)[0]
            keep.append(rows[np.argsort(idx[rows, 3], kind="stable")[:n]])    # the voxels nearest x = 0: a spatial crop
        keep = np.concatenate(keep)
        _CROPS[data] = (idx[keep], feats.cpu().numpy()[keep], shape)
    return _CROPS[data]


def _backbone(data):
    idx, f_np, shape = _cropped(data)
    torch.manual_seed(11)
    cls = spconv_backbone.VoxelResBackBone8x if data == "nus" else spconv_backbone.VoxelBackBone8x
    net = cls(AttrDict(), DATA[data][4], [shape[2], shape[1], shape[0] - 1]).to(DEV).train()
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty(m.num_features).uniform_(-0.3, 0.3, generator=g))
    return net, idx, f_np


def _forward(net, idx, f_np, fused):
    f = torch.from_numpy(f_np).to(DEV).requires_grad_(True)
    with spconv.fused_bn_train(fused):
        bd = net({"voxel_features": f, "voxel_coords": torch.from_numpy(idx).int().to(DEV), "batch_size": 2})
    taps = {k: bd["multi_scale_3d_features"]["x_" + k] for k in ("conv1", "conv2", "conv3", "conv4")}
    taps["conv_out"] = bd["encoded_spconv_tensor"]
    return f, taps


def _fused_nodes(t):
    """names of the autograd nodes below tensor t"""
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(n for n, _ in fn.next_functions)
    return names


@pytest.mark.parametrize("which", ["VoxelResBackBone8x-nus5", "VoxelBackBone8x-kitti4"])
def test_backbone_under_fused_bn_train_matches_fp64_replay(dev, which):
    """test_backbone_train_step_matches_fp64_replay with every BatchNorm1d (+ residual) + ReLU on the fused kernels: forward taps,
    input gradient and every parameter gradient against the fp64 Replay, held to the bounds that test holds the stock path to:
    1e-4 of each tensor's max |ref|, and 2e-2 for the gradients of VoxelResBackBone8x on the NuScenes crop, for the reason written
    there (the train-mode chain's ReLU gates on near-empty levels, not one kernel)."""
    data = "nus" if which.endswith("nus5") else "kitti"
    net, idx, f_np = _backbone(data)
    f, taps = _forward(net, idx, f_np, fused=True)
    names = _fused_nodes(taps["conv_out"].features)
    assert any("_BNReLURows" in n for n in names) and (data != "nus" or any("_BNAddReLURows" in n for n in names))
    assert not any("BatchNorm" in n for n in names), names             # no BatchNorm1d ran on torch
    loss = 0
    for t in taps.values():
        wts = _site_weights(t.indices.cpu().numpy(), t.features.shape[1])
        loss = loss + (t.features * torch.from_numpy(wts).float().to(DEV)).sum()
    loss.backward()
    rp = go.Replay()
    f_ref = torch.from_numpy(f_np).double().requires_grad_(True)
    rtaps = rp.backbone(net, f_ref, idx)
    rloss = 0
    errs = {}
    for name, t in taps.items():
        rf, ridx, rshape = rtaps[name]
        assert list(t.spatial_shape) == list(rshape), name
        gk, rk = sp._keys(t.indices.cpu().numpy(), rshape), sp._keys(ridx, rshape)
        assert np.array_equal(np.sort(gk), np.sort(rk)), f"{name}: active sites differ"
        wts = torch.from_numpy(_site_weights(ridx, rf.shape[1])).float().double()
        rloss = rloss + (rf * wts).sum()
        errs["fwd " + name] = _scaled_err(t.features[torch.from_numpy(np.argsort(gk)).to(DEV)], rf[torch.from_numpy(np.argsort(rk))])
    rloss.backward()
    errs["input grad"] = _scaled_err(f.grad, f_ref.grad)
    params = dict(net.named_parameters())
    for pname, p in params.items():
        assert p.grad is not None and rp.grad(p) is not None, pname
        if pname.endswith(("conv1.bias", "conv2.bias")):
            # a SparseBasicBlock conv bias feeds a train-mode BatchNorm: its gradient is 0 in exact arithmetic, so it is held to
            # the scale of the BatchNorm bias gradient it would have without the normalisation (as the stock-path test does)
            bn_bias = params[pname[:-len("conv1.bias")] + ("bn1.bias" if pname.endswith("conv1.bias") else "bn2.bias")]
            errs[pname] = float(p.grad.abs().max()) / float(rp.grad(bn_bias).abs().max())
        else:
            errs[pname] = _scaled_err(p.grad, rp.grad(p))
    worst = max(errs, key=errs.get)
    print(which, "fused rows", idx.shape[0], "worst", worst, f"{errs[worst]:.1e}",
          {k: f"{v:.1e}" for k, v in errs.items() if k.startswith("fwd") or k == "input grad"})
    bound = 2e-2 if data == "nus" else 1e-4
    assert all(v <= 1e-4 for k, v in errs.items() if k.startswith("fwd")), errs
    bad = {k: v for k, v in errs.items() if not v <= bound}
    assert not bad, bad


@pytest.mark.parametrize("data", ["kitti", "nus"])
def test_outside_fused_bn_train_nothing_changes(dev, data):
    """the stock grad-mode forward before the fused route was ever taken, inside fused_bn_train(False), and after a fused forward:
    the same autograd nodes (torch's BatchNorm, none of the fused ones) and the same bits in every tap and running statistic"""
    base, idx, f_np = _backbone(data)
    runs = []
    for fused in (None, False, True, None):
        net = copy.deepcopy(base)
        if fused is None:
            f = torch.from_numpy(f_np).to(DEV).requires_grad_(True)
            bd = net({"voxel_features": f, "voxel_coords": torch.from_numpy(idx).int().to(DEV), "batch_size": 2})
            taps = {k: bd["multi_scale_3d_features"]["x_" + k] for k in ("conv1", "conv2", "conv3", "conv4")}
            taps["conv_out"] = bd["encoded_spconv_tensor"]
        else:
            _, taps = _forward(net, idx, f_np, fused)
        names = _fused_nodes(taps["conv_out"].features)
        assert any("_BNReLURows" in n or "_BNAddReLURows" in n for n in names) == bool(fused), names
        assert any("BatchNorm" in n for n in names) != bool(fused), names
        if not fused:
            runs.append(([t.features.detach() for t in taps.values()], [b for k, b in net.named_buffers() if "running" in k]))
    for feats, stats in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(feats, runs[0][0]))
        assert all(torch.equal(a, b) for a, b in zip(stats, runs[0][1]))


# ---- 4. and 5. the model's step ------------------------------------------------------------------------------------------------
NOISE = 2.0 ** -17       # the noise floor of tests/test_gpu_bev_train.py's fused-against-stock comparisons (reasoned there)


def _second_inputs(B, seed):
    """clouds of 4000 points per frame and 4 gt boxes in every frame but the last, which has none"""
    r = np.random.default_rng(seed)
    frames = []
    for i in range(B):
        c = synth.cloud_ring(2400 + seed + i)
        frames.append(c[np.sort(r.permutation(len(c))[:4000])])
    pts = torch.from_numpy(np.concatenate(frames)).to(DEV)
    offs = torch.tensor(np.cumsum([0] + [len(f) for f in frames]), dtype=torch.int32, device=DEV)
    gt = np.zeros((B, 6, 8), np.float32)
    size = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    for b in range(B - 1):
        n = 4
        cls = np.array([1, 2, 3, 1])
        gt[b, :n, 0], gt[b, :n, 1], gt[b, :n, 2] = r.uniform(5, 60, n), r.uniform(-30, 30, n), r.uniform(-1.5, -0.5, n)
        gt[b, :n, 3:6] = size[cls - 1] * r.uniform(0.9, 1.1, (n, 1))
        gt[b, :n, 6], gt[b, :n, 7] = r.uniform(-np.pi, np.pi, n), cls
    return pts, offs, torch.from_numpy(gt).to(DEV)


def _second_models(n):
    from lidardetection_amd.second import SECONDKitti
    models = []
    for _ in range(n):
        torch.manual_seed(6)
        models.append(SECONDKitti(batch_size=2, max_voxels=2000, device=DEV).train())
    return models


def _capture_dense_part(model):
    """records the BEV map entering backbone_head_stock and its (cls, box, dirs) outputs, whose gradients are retained"""
    orig, box = model.backbone_head_stock, {}

    def wrapped(c):
        out = orig(c)
        for t in out:
            t.retain_grad()
        box["canvas"], box["heads"] = c.detach(), out
        return out
    model.backbone_head_stock = wrapped
    return box


def _dense_replay_grads(model, canvas, head_grads):
    """the dense part (blocks, deblocks, heads; train-mode BatchNorm2d) replayed in float64 on the CPU from the BEV map `canvas`,
    backward from the gradients of the three head outputs -> {parameter name: float64 gradient}"""
    names = ("blocks", "deblocks", "conv_cls", "conv_box", "conv_dir_cls")
    mods = {n: copy.deepcopy(getattr(model, n)).cpu().double().train() for n in names}
    for m in mods.values():
        for p in m.parameters():
            p.grad = None
    x, ups = canvas.cpu().double().contiguous(), []
    for blk, de in zip(mods["blocks"], mods["deblocks"]):
        x = blk(x)
        ups.append(de(x))
    cat = torch.cat(ups, 1)
    outs = [mods[n](cat).permute(0, 2, 3, 1).reshape(canvas.shape[0], -1, k) for n, k in (("conv_cls", 3), ("conv_box", 7), ("conv_dir_cls", 2))]
    torch.autograd.backward(outs, [g.cpu().double() for g in head_grads])
    return {f"{n}.{k}": p.grad for n, m in mods.items() for k, p in m.named_parameters()}


def test_second_train_loss_fused_matches_stock(dev):
    """sparse="fused", backbone="fused" against "stock", "stock" on identical weights: the three losses (rtol 1e-4) and every
    parameter's gradient, by the criterion of test_gpu_bev_train.test_train_loss_fused_matches_stock_and_refolds: within
    max(1e-4, 10 x the stock step's own spread under a 2^-17 relative perturbation of the BEV map) of the tensor's scale.  The loss
    head's anchors are the model's.

    A tensor beyond that bound is measured, in both paths, against a float64 CPU replay of the dense part, and the fused path is
    held to at most twice the stock path's error.  Measured on an MI355X: one tensor takes that route, deblocks.0.0.weight (fused
    against stock 1.9e-3 of its scale, spread 1.2e-4); against the replay the fused path is at 1.2e-4 and the stock path at 1.9e-3
    (its fp32 BatchNorm backward over the 70 400 pixels of the 200 x 176 map).  The replay costs about 15 s of CPU time."""
    pts, offs, gt = _second_inputs(2, 5)
    fused, stock, noisy = _second_models(3)
    head = fused._loss_head()
    assert head.loss_anchors().shape == fused.anchors.shape and torch.equal(head.loss_anchors(), fused.anchors)
    orig = noisy.backbone_head_stock
    g = torch.Generator().manual_seed(9)
    noisy.backbone_head_stock = lambda c: orig(c * (1 + NOISE * torch.randn(c.shape, generator=g).to(DEV).contiguous(memory_format=CL)))
    cap = _capture_dense_part(stock)
    lf = fused.train_loss(pts, offs, gt, backbone="fused", sparse="fused")
    ls = stock.train_loss(pts, offs, gt)
    ln = noisy.train_loss(pts, offs, gt)
    print("losses fused", [float(a.detach()) for a in lf], "stock", [float(a.detach()) for a in ls])
    for a, b in zip(lf, ls):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    for ll in (lf, ls, ln):
        sum(ll).backward()
    pf, ps, pn = dict(fused.named_parameters()), dict(stock.named_parameters()), dict(noisy.named_parameters())
    errs = {k: rel(p.grad, ps[k].grad, empty_ok=True) for k, p in pf.items() if p.grad is not None}
    assert len(errs) == len(ps)
    floors = {k: rel(pn[k].grad, ps[k].grad, empty_ok=True) for k in errs}
    worst = max(errs, key=lambda k: errs[k] / max(1e-4, 10 * floors[k]))
    print("worst", worst, f"{errs[worst]:.1e}", "floor", f"{floors[worst]:.1e}")
    bad = {k: (v, floors[k]) for k, v in errs.items() if not v < max(1e-4, 10 * floors[k])}
    if bad:
        # a tensor beyond that bound: both paths against the float64 CPU replay of the dense part (from the stock step's BEV map and
        # head-output gradients); the fused path is held to at most twice the stock path's error
        assert all(k.startswith(("blocks.", "deblocks.", "conv_")) for k in bad), bad
        rep = _dense_replay_grads(stock, cap["canvas"], [t.grad for t in cap["heads"]])
        vs64 = {k: (rel(pf[k].grad, rep[k], empty_ok=True), rel(ps[k].grad, rep[k], empty_ok=True)) for k in bad}
        print("beyond the stock-spread bound", bad, "against the fp64 replay (fused, stock)", vs64)
        worse = {k: v for k, v in vs64.items() if not v[0] <= 2 * v[1]}
        assert not worse, (worse, bad)
    for (k, bf), bs in zip(fused.named_buffers(), stock.buffers()):
        if "running" in k:
            torch.testing.assert_close(bf, bs, rtol=1e-5, atol=1e-6)
        elif "num_batches" in k:
            assert int(bf) == int(bs) == 1


def test_second_train_step_two_iterations(dev):
    from lidardetection_amd import optim
    from lidardetection_amd.pointpillar import PointPillarKITTI
    from lidardetection_amd.second import SECONDKitti
    assert SECONDKitti.train_step is PointPillarKITTI.train_step     # inherited
    pts, offs, gt = _second_inputs(2, 17)
    (model,) = _second_models(1)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    stats = {k: b.detach().clone() for k, b in model.named_buffers() if "running" in k and k.startswith("backbone3d")}
    opt = optim.AdamOneCycle(model, wd=0.01, max_grad_norm=10.0)
    for it in range(2):
        opt.lr, opt.mom = optim.one_cycle(it, 10)
        out = model.train_step(pts, offs, gt, opt, sparse="fused", backbone="fused")
        assert len(out) == 4 and all(t.is_cuda and not t.requires_grad and bool(torch.isfinite(t).all()) for t in out)
        print("step", it, [float(t) for t in out])
    for part in ("backbone3d.", "blocks.", "deblocks.", "conv_cls.", "conv_box.", "conv_dir_cls."):
        moved = [k for k, p in model.named_parameters() if k.startswith(part) and not torch.equal(p.detach(), before[k])]
        total = [k for k in before if k.startswith(part)]
        assert total and len(moved) == len(total), (part, sorted(set(total) - set(moved)))
    assert stats and all(not torch.equal(b, stats[k]) for k, b in model.named_buffers() if k in stats)
