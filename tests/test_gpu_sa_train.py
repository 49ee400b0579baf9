"""GPU checks of the train-mode set-abstraction kernels (csrc/sa_train.hip) against the float64 replay of
tests/_sa_train_np.py fed the device's idx and arg, and of StackSAModuleMSG under sa_train.fused_sa_train().

Tolerance: the project's train-kernel bound, 1e-4 of each tensor's max |reference| (tests/test_gpu_second_train.py).  Elements whose
float64 pre-activation lies within 1e-6 of zero are excluded (the ReLU mask may legitimately differ there); at most 1e-3 of the
elements may be excluded."""
import copy

import numpy as np
import pytest
import torch

import _sa_train_np as ref
from lidardetection_amd import sa_train
from lidardetection_amd.ext import pointnet2_stack_cuda as native
from lidardetection_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pn_modules

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, NEAR0, MAX_EXCLUDED = 1e-4, 1e-6, 1e-3
EPS = 1e-5


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _close(got, want, what, keep=None):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    err = np.abs(got - want)
    if keep is not None:
        err = err * keep
    scale = max(float(np.abs(want).max()), 1e-30)
    print(what, f"max err {err.max() / scale:.2e} of scale {scale:.3e}")
    assert err.max() <= TOL * scale, (what, err.max() / scale)


def _device_case(case):
    seed, xyz_cnt, new_cnt, ns, H, radius = case
    xyz, feats, new_xyz = ref.cloud(seed, xyz_cnt, new_cnt, 5)
    xc, nc = _t(xyz_cnt, torch.int32), _t(new_cnt, torch.int32)
    idx = torch.zeros((len(new_xyz), ns), dtype=torch.int32, device=DEV)
    native.ball_query_wrapper(len(xyz_cnt), len(new_xyz), radius, ns, _t(new_xyz), nc, _t(xyz), xc, idx)
    return xyz, feats, new_xyz, xc, nc, idx


@pytest.mark.parametrize("case", ref.CASES, ids=[f"seed{c[0]}-ns{c[3]}-H{c[4]}" for c in ref.CASES])
def test_gather_and_inverse_index(dev, case):
    seed, xyz_cnt, new_cnt, ns, H, radius = case
    xyz, _, new_xyz, xc, nc, idx = _device_case(case)
    idx_h = idx.cpu().numpy()
    host_idx = ref.ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, ns)
    print("balls: empty", int((idx_h[:, 0] < 0).sum()), "of", len(idx_h), "| equal to the host ball query:", bool((host_idx == idx_h).all()))
    N, M = len(xyz), len(new_xyz)
    r = np.random.default_rng(seed + 100)
    table, query = r.standard_normal((N, H)).astype(np.float32), r.standard_normal((M, H)).astype(np.float32)
    dz = r.standard_normal((M * ns, H)).astype(np.float32)
    for q in (query, None):
        qd = None if q is None else _t(q)
        z = sa_train.sa_gather_forward(_t(table), qd, idx, xc, nc)
        want = ref.gather_forward(table, q, idx_h, xyz_cnt, new_cnt)
        _close(z, want, "z")
        empty_rows = np.repeat(idx_h[:, 0] < 0, ns)
        assert not z.cpu().numpy()[empty_rows].any()                     # exactly 0 (also no -0.0 bits set)
        assert torch.equal(z, sa_train.sa_gather_forward(_t(table), qd, idx, xc, nc))
    row_start, pairs = sa_train.inverse_index(idx, xc, nc, N)
    rs_ref, pairs_ref = ref.inverse_index(idx_h, xyz_cnt, new_cnt, N)
    assert row_start.dtype == pairs.dtype == torch.int32
    assert np.array_equal(row_start.cpu().numpy(), rs_ref) and np.array_equal(pairs.cpu().numpy(), pairs_ref)
    again = sa_train.inverse_index(idx, xc, nc, N)
    assert torch.equal(again[0], row_start) and torch.equal(again[1], pairs)
    d_table, d_query = sa_train.sa_gather_backward(_t(dz), idx, row_start, pairs, N)
    dt_ref, dq_ref = ref.gather_backward(dz, idx_h, xyz_cnt, new_cnt, N)
    _close(d_table, dt_ref, "d_table")
    _close(d_query, dq_ref, "d_query")
    t2, q2 = sa_train.sa_gather_backward(_t(dz), idx, row_start, pairs, N)
    assert torch.equal(t2, d_table) and torch.equal(q2, d_query)
    assert sa_train.sa_gather_backward(_t(dz), idx, row_start, pairs, N, need_query=False)[1] is None
    # through autograd
    tt, qq = _t(table).requires_grad_(), _t(query).requires_grad_()
    sa_train.sa_gather_train(tt, qq, idx, xc, nc).backward(_t(dz))
    assert torch.equal(tt.grad, d_table) and torch.equal(qq.grad, d_query)


@pytest.mark.parametrize("case", ref.CASES, ids=[f"seed{c[0]}-ns{c[3]}-H{c[4]}" for c in ref.CASES])
def test_bn_relu_max(dev, case):
    """case 1 has M * nsample = 8 rows; gamma has negative channels (the maximum of y then sits at the minimum of z); rows of some
    queries are duplicated (exact ties) and a quarter of the queries are all-zero rows (an empty ball's).  Query 0 is never one of
    those: at M = 1 the batch would otherwise have zero variance, where 1 / sqrt(eps) amplifies the fp32 rounding of scale and shift
    beyond any bound stated relative to the output."""
    seed, _, new_cnt, ns, H, _ = case
    M = int(sum(new_cnt))
    if M * ns < 2:
        M = 2
    r = np.random.default_rng(seed + 200)
    z = (r.standard_normal((M, ns, H)) * 1.5 + 0.3).astype(np.float32)
    if ns > 1:
        z[1::3, 1:] = z[1::3, :1]                                         # a padded ball: every sample is the first hit
    z[2::4] = 0                                                            # empty balls
    z = z.reshape(M * ns, H)
    gamma = r.uniform(0.5, 1.5, H).astype(np.float32) * np.where(np.arange(H) % 3 == 1, -1, 1).astype(np.float32)
    beta = r.uniform(-0.5, 0.5, H).astype(np.float32)
    g = r.standard_normal((M, H)).astype(np.float32)
    zd, gd, bd = _t(z), _t(gamma), _t(beta)
    out, arg, stats, scale_shift, batch_stats = sa_train.bn_relu_max_forward(zd, M, ns, gd, bd, EPS)
    run2 = sa_train.bn_relu_max_forward(zd, M, ns, gd, bd, EPS)
    assert all(torch.equal(a, b) for a, b in zip((out, arg, stats, scale_shift, batch_stats), run2))
    arg_h = arg.cpu().numpy()
    assert arg.dtype == torch.uint8 and int(arg_h.max()) < ns
    want, y64, pre, (mu, var, var_u) = ref.bn_relu_max_forward(z, M, ns, gamma, beta, EPS, arg_h)
    # arg on its own: the chosen sample's float64 y within 1e-5 of scale of the float64 maximum ...
    scale = max(float(y64.max()), 1e-30)
    assert float((y64.max(1) - want).max()) <= 1e-5 * scale
    # ... and the lowest index whenever the fp32 values tie exactly (fp32 y restated from the device's scale / shift)
    ss = scale_shift.cpu().numpy().astype(np.float64)
    y32 = np.maximum((z.astype(np.float64) * ss[:H] + ss[H:]).astype(np.float32), 0).reshape(M, ns, H)
    assert np.array_equal(arg_h, np.argmax(y32, axis=1))
    near = np.abs(np.take_along_axis(pre, arg_h.astype(np.int64)[:, None, :], 1)[:, 0]) < NEAR0          # (M, H)
    print("excluded", int(near.sum()), "of", near.size)
    assert near.mean() <= MAX_EXCLUDED
    _close(out, want, "out", keep=~near)
    bs = batch_stats.double().cpu().numpy()
    _close(batch_stats[:H], mu, "mean")
    np.testing.assert_allclose(bs[H:2 * H], var, rtol=1e-5)
    np.testing.assert_allclose(bs[2 * H:], var_u, rtol=1e-5)
    dz, d_gamma, d_beta = sa_train.bn_relu_max_backward(zd, M, ns, _t(g), arg, gd, stats, scale_shift)
    run2 = sa_train.bn_relu_max_backward(zd, M, ns, _t(g), arg, gd, stats, scale_shift)
    assert all(torch.equal(a, b) for a, b in zip((dz, d_gamma, d_beta), run2))
    dz_ref, dg_ref, db_ref = ref.bn_relu_max_backward(z, M, ns, g, arg_h, gamma, beta, EPS)
    chan_ok = ~near.any(0)
    _close(dz, dz_ref, "dz", keep=np.broadcast_to(chan_ok, dz_ref.shape))
    _close(d_gamma, dg_ref, "d_gamma", keep=chan_ok)
    _close(d_beta, db_ref, "d_beta", keep=chan_ok)


# ---- the module ----------------------------------------------------------------------------------------------------------------------
def _module(mlps, radii, nsamples, seed):
    torch.manual_seed(seed)
    m = pn_modules.StackSAModuleMSG(radii=radii, nsamples=nsamples, mlps=[list(w) for w in mlps], use_xyz=True, pool_method='max_pool')
    m = m.to(DEV).train()
    with torch.no_grad():
        for k, p in m.named_parameters():                                   # BatchNorm away from its identity initialisation
            if p.dim() == 1:
                p.copy_(torch.rand_like(p) + (0.5 if k.endswith("weight") else -0.5))
    return m


def _module_inputs(seed, xyz_cnt, new_cnt, width):
    xyz, feats, new_xyz = ref.cloud(seed, xyz_cnt, new_cnt, width)
    return xyz, feats, new_xyz, _t(xyz_cnt, torch.int32), _t(new_cnt, torch.int32)


MODULES = [   # PV-RCNN's widths: the raw-point layer, the x_conv3 layer, the RoI-grid pool
    ("raw", [[1, 16, 16], [1, 16, 16]], [0.4, 0.8], [16, 16], 1),
    ("x_conv3", [[64, 64, 64], [64, 64, 64]], [1.2, 2.4], [16, 32], 64),
    ("roi_grid", [[128, 64, 64], [128, 64, 64]], [0.8, 1.6], [16, 16], 128),
]


@pytest.mark.parametrize("name,mlps,radii,nsamples,width", MODULES, ids=[m[0] for m in MODULES])
def test_module_fused_against_replay(dev, monkeypatch, name, mlps, radii, nsamples, width):
    xyz_cnt, new_cnt = [150, 0, 90], [40, 30, 0]
    xyz, feats, new_xyz, xc, nc = _module_inputs(11, xyz_cnt, new_cnt, width)
    mod = _module(mlps, radii, nsamples, 3)
    stock = copy.deepcopy(mod)
    args_seen, orig = [], sa_train.bn_relu_max_forward

    def capture(*a, **k):
        res = orig(*a, **k)
        args_seen.append(res[1])
        return res
    monkeypatch.setattr(sa_train, "bn_relu_max_forward", capture)
    f = _t(feats).requires_grad_()
    with sa_train.fused_sa_train():
        _, out = mod(xyz=_t(xyz), xyz_batch_cnt=xc, new_xyz=_t(new_xyz), new_xyz_batch_cnt=nc, features=f)
    assert len(args_seen) == len(mlps), "the fused route did not run"
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    out.backward(gout)
    with torch.no_grad():
        idxs = mod._ball_queries(_t(xyz), xc, _t(new_xyz), nc)
    c0 = 0
    d_feats = np.zeros((len(xyz), width))
    for k, (mlp, idx, arg) in enumerate(zip(mod.mlps, idxs, args_seen)):
        mods = list(mlp)
        Ws = [c.weight.detach()[:, :, 0, 0].cpu().numpy() for c in mods[0::3]]
        Gs = [b.weight.detach().cpu().numpy() for b in mods[1::3]]
        Bs = [b.bias.detach().cpu().numpy() for b in mods[1::3]]
        h = Ws[-1].shape[0]
        rep = ref.scale_replay(xyz, feats, new_xyz, idx.cpu().numpy(), xyz_cnt, new_cnt, Ws, Gs, Bs, mods[1].eps,
                               gout[:, c0:c0 + h].cpu().numpy(), arg.cpu().numpy())
        assert (np.abs(rep["pre_last"]) < NEAR0).mean() <= MAX_EXCLUDED
        _close(out[:, c0:c0 + h], rep["out"], f"{name} scale {k} out")
        for j, (conv, bn) in enumerate(zip(mods[0::3], mods[1::3])):
            _close(conv.weight.grad[:, :, 0, 0], rep["d_w"][j], f"{name} scale {k} dW{j}")
            _close(bn.weight.grad, rep["d_gamma"][j], f"{name} scale {k} dgamma{j}")
            _close(bn.bias.grad, rep["d_beta"][j], f"{name} scale {k} dbeta{j}")
        d_feats += rep["d_feats"]
        c0 += h
    _close(f.grad, d_feats, f"{name} d_features")
    # running statistics: the stock module's, to 1e-5
    _, out_s = stock(xyz=_t(xyz), xyz_batch_cnt=xc, new_xyz=_t(new_xyz), new_xyz_batch_cnt=nc, features=_t(feats))
    _close(out, out_s.detach().cpu().numpy(), f"{name} out against the stock route")
    for (k, bf), bs in zip(mod.named_buffers(), stock.buffers()):
        if "running" in k:
            torch.testing.assert_close(bf, bs, rtol=1e-5, atol=1e-5)
        else:
            assert int(bf) == int(bs) == 1


def _parent_route(mod, xyz, xc, new_xyz, nc, feats, keep=None):
    """StackSAModuleMSG.forward's stock body as the parent commit runs it; keep: a list that receives every scale's grouped tensor
    with its gradient retained"""
    from lidardetection_amd.pcdet.ops.pointnet2 import _common as C
    per_scale = []
    for grouper, mlp in zip(mod.groupers, mod.mlps):
        grouped, _ = grouper(xyz, xc, new_xyz, nc, feats)
        if keep is not None:
            grouped.retain_grad()
            keep.append(grouped)
        y = mlp(grouped.permute(1, 0, 2).unsqueeze(0))
        per_scale.append(C.pool_over_samples(y, mod.pool_method)[0].t())
    return torch.cat(per_scale, dim=1)


def _graph(t):
    """the autograd graph behind `t` as the list of its node types, depth first: the computation a backward pass will run"""
    names, stack, seen = [], [t.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


@pytest.fixture
def deterministic_library():
    """the library convolutions and BatchNorm in their deterministic mode, no solver search; restored afterwards"""
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was


def _atomic_sum_bound(grouped_grad, idx_raw, xyz_cnt, new_cnt, N):
    """How far two evaluations of the grouping gradient may differ per element.  d_features[n, c] is the fp32 sum, by atomicAdd in
    no fixed order, of the k addends grouped_grad[m, 3 + c, s] over the pairs that read source n.  Any order of a k-term fp32 sum is
    within gamma_(k-1) * sum |addends| of the exact sum (gamma_j = j u / (1 - j u), u = 2^-24; Higham, Accuracy and Stability of
    Numerical Algorithms, (4.4)), so two orders are within twice that of each other.  -> (N, C) float64"""
    g = np.abs(grouped_grad[:, 3:, :].double().cpu().numpy()).transpose(0, 2, 1)         # (M, ns, C)
    key = ref.pair_keys(idx_raw, xyz_cnt, new_cnt, N)
    live = key < N
    total, count = np.zeros((N, g.shape[2])), np.zeros(N)
    np.add.at(total, key[live], g.reshape(-1, g.shape[2])[live])
    np.add.at(count, key[live], 1)
    j = np.maximum(count - 1, 0) * 2.0 ** -24
    return 2 * (j / (1 - j))[:, None] * total


@pytest.mark.parametrize("how", ["outside", "inside_unsupported"])
def test_stock_route_unchanged(dev, deterministic_library, how):
    """outside fused_sa_train(), and inside it for a module that does not qualify (a width of 6), forward() is the parent commit's
    route bit for bit: the output, the buffers, the autograd graph node for node, every parameter gradient at nsample 1 and 8, and
    the feature gradient at nsample 1 (one addend per source and pair: no order to vary).

    At nsample 8 the feature gradient is the grouping kernel's float atomicAdd of several addends per source, whose order is not
    fixed run to run (14 - 16 bit patterns in 16 runs of the parent's route on an MI355X, where the output and every parameter
    gradient always had one).  Bit identity cannot hold there for any code, the parent's included, so each element is held to the
    bound that reordering its own addends allows (_atomic_sum_bound), computed from the addends themselves, not from another run."""
    mlps = [[8, 16, 16]] if how == "outside" else [[8, 6, 16]]
    xyz_cnt, new_cnt = [120, 80], [30, 25]
    N = sum(xyz_cnt)
    for nsample in (1, 8):
        xyz, feats, new_xyz, xc, nc = _module_inputs(21, xyz_cnt, new_cnt, 8)
        a = _module(mlps, [0.9], [nsample], 4)
        warm, b = copy.deepcopy(a), copy.deepcopy(a)
        fa, fw, fb = (_t(feats).requires_grad_() for _ in range(3))
        gout = torch.randn((sum(new_cnt), 16), generator=torch.Generator().manual_seed(6)).to(DEV)
        _parent_route(warm, _t(xyz), xc, _t(new_xyz), nc, fw).backward(gout)     # the library has picked its kernels for these shapes
        with sa_train.fused_sa_train(how != "outside"):
            assert how == "outside" or not sa_train.module_supported(a)
            _, out = a(xyz=_t(xyz), xyz_batch_cnt=xc, new_xyz=_t(new_xyz), new_xyz_batch_cnt=nc, features=fa)
        kept = []
        want = _parent_route(b, _t(xyz), xc, _t(new_xyz), nc, fb, keep=kept)
        assert torch.equal(out, want)
        assert _graph(out) == _graph(want)
        out.backward(gout)
        want.backward(gout)
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p.grad, q.grad), (k, nsample, float((p.grad - q.grad).abs().max()))
        for p, q in zip(a.buffers(), b.buffers()):
            assert torch.equal(p, q)
        if nsample == 1:
            assert torch.equal(fa.grad, fb.grad)
            continue
        with torch.no_grad():
            (idx_raw,) = b._ball_queries(_t(xyz), xc, _t(new_xyz), nc)
        bound = _atomic_sum_bound(kept[0].grad, idx_raw.cpu().numpy(), xyz_cnt, new_cnt, N)
        diff = (fa.grad - fb.grad).abs().double().cpu().numpy()
        print("feature gradient, nsample 8: elements that differ", int((diff > 0).sum()), "of", diff.size, "| worst diff / bound",
              float((diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all()
