"""GPU checks of the train-path kernels over the ranges include/lidar_hip.h declares, each against a plain float64 reference of the
same operation: csrc/pfn_train.hip (train-mode PillarVFE, scatter backward), csrc/bn_train.hip (batch-statistics BatchNorm2d + ReLU,
through the raw entry points so that x_off / y_off / g_off are really passed) and csrc/wino43_wgrad.hip (rectangular widths,
x_ld != g_ld, every small map, the 512-tile split).  The other train-path files test these kernels at production points.

Every input is drawn on the CPU from a seeded generator, so the preconditions that are asserted on the float64 reference (no
near-tie between a pillar's two best rows, no pre-activation within 1e-5 of the ReLU edge) hold for the committed seeds on any
machine.  Those preconditions bound what a PFN case can hold: a near-tie has a probability of ~1e-3 per (pillar, channel) at
20..64 points, so the cases with many points keep V * cout below ~1000 and the large V come with one or two points per pillar.
Every value of every axis of the sweep still appears."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from _gpu_util import rel, release_memory  # noqa: F401  (release_memory: an autouse fixture)
from lidardetection_amd import _lib, pillar_ops
from lidardetection_amd.pcdet.models.backbones_3d.vfe.encoders import PillarVFE
from lidardetection_amd.pcdet.utils.cfg import AttrDict
from test_gpu_wino_wgrad import BAR, _ref64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 777.0


# ------------------------------------------------------------------ 1. PFN train (csrc/pfn_train.hip)
PFN_VOXEL, PFN_RANGE = (2.0, 2.0, 4.0), (0.0, -8.0, -3.0, 16.0, 8.0, 1.0)          # an 8 x 8 grid of pillars
PFN_NX = PFN_NY = 8

# (num_features, with_distance, max_points, cout, V): every value of every axis, the corners (8, dist, 64, 64) and (3, -, 1, 1)
PFN_SWEEP = [
    (8, 1, 64, 64, 3), (3, 0, 1, 1, 257), (4, 0, 20, 3, 255), (5, 1, 33, 1, 257), (6, 0, 63, 16, 1), (7, 1, 1, 16, 4001),
    (6, 1, 2, 60, 3), (7, 0, 64, 1, 255), (3, 1, 20, 32, 3), (4, 1, 63, 60, 1), (5, 0, 1, 64, 255), (8, 0, 33, 32, 1),
    (3, 0, 2, 3, 257),
]
# the variants of the issue, on a subset: (sweep point, seed, keyword arguments of _pfn_case)
PFN_VARIANTS = {
    "float_coords_counts_corner": ((8, 1, 64, 64, 3), dict(as_float=True)),
    "float_coords_counts_blocks": ((4, 0, 20, 3, 255), dict(as_float=True)),
    "device_count_poisoned_tail": ((4, 0, 20, 3, 255), dict(tail=45)),
    "device_count_poisoned_tail_float": ((5, 1, 2, 16, 33), dict(tail=31, as_float=True)),
    "gammas_negative": ((7, 1, 20, 16, 3), dict(gammas="neg")),
    "gammas_1e-3_both_signs": ((6, 0, 33, 16, 3), dict(gammas="tiny")),
    "gammas_negative_cout60": ((5, 0, 2, 60, 33), dict(gammas="neg")),
    "duplicate_points": ((4, 0, 20, 64, 40), dict(dup=True)),
    "duplicate_points_dist_full_wave": ((8, 1, 64, 60, 9), dict(dup=True, gammas="neg")),
}


def _pfn_inputs(cfg, seed, dup=False):
    """CPU tensors: voxels (V, P, C) with zero padded slots, counts (V,) in [1, P] (pillar 0 full, pillar 1 a single point when
    V >= 2; no pillar is empty), coords (V, 4) [b, z, y, x]"""
    C_, dist, P, cout, V = cfg
    g = torch.Generator(device="cpu").manual_seed(seed)
    num = torch.randint(1, P + 1, (V,), generator=g, dtype=torch.int32)
    num[0::3] = P                                                    # full pillars: no padded row in the max
    if V >= 2:
        num[1::3] = 1
    cells = torch.randint(0, PFN_NX, (V, 2), generator=g, dtype=torch.int32)
    coords = torch.stack([torch.zeros(V, dtype=torch.int32), torch.zeros(V, dtype=torch.int32), cells[:, 0], cells[:, 1]], 1)
    u = torch.rand((V, P, C_), generator=g)
    vs, rg = torch.tensor(PFN_VOXEL), torch.tensor(PFN_RANGE[:3])
    origin = coords[:, [3, 2, 1]].float() * vs + rg
    vox = u.clone()
    vox[:, :, :3] = origin.unsqueeze(1) + u[:, :, :3] * vs
    if dup:                                                          # the second half of a pillar's points repeats the first
        for v in range(V):
            n = int(num[v])
            h = n // 2
            if h:
                vox[v, h:2 * h] = vox[v, :h]
    real = torch.arange(P).view(1, -1) < num.view(-1, 1)
    return (vox * real.unsqueeze(-1)).contiguous(), num, coords.contiguous()


def _pfn_module(cfg, seed, gammas="mixed"):
    C_, dist, P, cout, V = cfg
    torch.manual_seed(seed)
    m = PillarVFE(AttrDict(dict(USE_NORM=True, WITH_DISTANCE=bool(dist), USE_ABSLOTE_XYZ=True, NUM_FILTERS=[cout])), C_, PFN_VOXEL,
                  PFN_RANGE)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    with torch.no_grad():
        bn = m.pfn_layers[0].norm
        gm = torch.empty(cout).uniform_(0.3, 1.5, generator=g)
        if gammas == "mixed":
            gm[::3] *= -1
        elif gammas == "neg":
            gm *= -1
        elif gammas == "tiny":                                       # magnitude 1e-3, both signs
            gm = 1e-3 * (1 + 0.5 * (gm - 0.9))
            gm[1::2] *= -1
        bn.weight.copy_(gm)
        bn.bias.copy_(torch.empty(cout).normal_(0, 0.3, generator=g))
        bn.running_mean.copy_(torch.empty(cout).uniform_(-0.2, 0.2, generator=g))
        bn.running_var.copy_(torch.empty(cout).uniform_(0.8, 1.2, generator=g))
    return m.train()


def pfn_preconditions(ref, vox64, num, coords, dup):
    """on the float64 reference alone -> (smallest gap between the two best candidates / max |z|, smallest |BN(z_sel)|).  The
    candidates of a (pillar, channel) are its real rows and, when n < P, ONE padded row (z = 0)."""
    layer = ref.pfn_layers[0]
    V, P, _ = vox64.shape
    z = F.linear(ref._decorate(vox64, num, coords), layer.linear.weight).detach()      # (V, P, cout), padded rows 0
    gamma, beta = layer.norm.weight.detach(), layer.norm.bias.detach()
    mu, var = z.mean(dim=(0, 1)), z.var(dim=(0, 1), unbiased=False)
    sign = torch.where(gamma < 0, -1.0, 1.0).to(z.dtype)
    zs = z * sign                                                                       # the selected row maximises zs
    real = (torch.arange(P, device=z.device).view(1, -1) < num.view(-1, 1)).unsqueeze(-1)
    ninf = torch.full_like(zs[:, :1], float("-inf"))
    pad = torch.where((num < P).view(-1, 1, 1), torch.zeros_like(ninf), ninf)
    cand = torch.cat([torch.where(real, zs, ninf.expand_as(zs)), pad, ninf], dim=1)
    top = cand.topk(2, dim=1).values
    gap = float(((top[:, 0] - top[:, 1]) / z.abs().max()).min())
    bn = gamma * (top[:, 0] * sign - mu) / torch.sqrt(var + layer.norm.eps) + beta
    return (float("inf") if dup else gap), float(bn.abs().min())


def _pfn_case(cfg, seed, as_float=False, tail=0, gammas="mixed", dup=False, dev=None, check_only=False):
    """one configuration against the mirror's stock PillarVFE in float64 (train mode): out, batch statistics, the running statistics
    after one and two calls, d_weight / d_gamma / d_beta.  Pillars with n == 0 are excluded: the reference divides by the count."""
    dev = DEV if dev is None else dev
    C_, dist, P, cout, V = cfg
    vox, num, coords = (t.to(dev) for t in _pfn_inputs(cfg, seed, dup))
    ref = _pfn_module(cfg, seed, gammas).to(dev).double()
    gap, edge = pfn_preconditions(ref, vox.double(), num, coords, dup)
    print(f"pfn {cfg} seed {seed}: gap / max|z| {gap:.3e}, min |BN(zsel)| {edge:.3e}")
    assert gap > 1e-4 and edge > 1e-5, (gap, edge)
    if check_only:
        return
    m = _pfn_module(cfg, seed, gammas).to(dev)
    layer, rl = m.pfn_layers[0], ref.pfn_layers[0]
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    grad = torch.randn((V, cout), generator=g).to(dev)
    nvd = None
    kv, kn, kc, kg = vox, num, coords, grad
    if tail:                                                         # rows past the device count: poisoned, neither read nor counted
        kv = torch.cat([vox, torch.full((tail, P, C_), float("nan"), device=dev)])
        kn = torch.cat([num, torch.full((tail,), -3, dtype=torch.int32, device=dev)])
        kc = torch.cat([coords, torch.full((tail, 4), -7, dtype=torch.int32, device=dev)])
        kg = torch.cat([grad, torch.full((tail, cout), 3.0, device=dev)])
        nvd = torch.tensor([V], dtype=torch.int32, device=dev)
    if as_float:
        kn, kc = kn.float(), kc.float()
    call = lambda: pillar_ops.pillar_vfe_train(kv, kn, kc, layer.linear.weight, layer.norm.weight, layer.norm.bias,      # noqa: E731
                                               layer.norm.running_mean, layer.norm.running_var, PFN_VOXEL, PFN_RANGE,
                                               with_distance=bool(dist), num_batches_tracked=layer.norm.num_batches_tracked,
                                               num_voxels_dev=nvd, return_stats=True)
    out, mean, var = call()
    (out * kg).sum().backward()
    bd = {"voxels": vox.double(), "voxel_num_points": num, "voxel_coords": coords}
    want = ref(dict(bd))["pillar_features"].reshape(V, cout)
    (want * grad.double()).sum().backward()
    z = F.linear(ref._decorate(vox.double(), num, coords), rl.linear.weight).detach()
    if tail:
        assert out.shape[0] == V + tail and bool((out[V:] == 0).all())
    errs = {"out": rel(out[:V], want)}
    assert errs["out"] < 1e-5, errs
    mean64, var64 = z.mean(dim=(0, 1)), z.var(dim=(0, 1), unbiased=False)
    torch.testing.assert_close(mean.double(), mean64, rtol=1e-6, atol=1e-6 * float(mean64.abs().max()))
    torch.testing.assert_close(var.double(), var64, rtol=1e-6, atol=0)
    torch.testing.assert_close(layer.norm.running_mean.double(), rl.norm.running_mean, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(layer.norm.running_var.double(), rl.norm.running_var, rtol=1e-6, atol=0)
    for name, a, b in (("d_weight", layer.linear.weight, rl.linear.weight), ("d_gamma", layer.norm.weight, rl.norm.weight),
                       ("d_beta", layer.norm.bias, rl.norm.bias)):
        assert a.grad is not None and bool(torch.isfinite(a.grad).all()), name
        errs[name] = rel(a.grad, b.grad)
    print(f"pfn {cfg} seed {seed}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(errs[k] < 1e-4 for k in ("d_weight", "d_gamma", "d_beta")), errs
    with torch.no_grad():                                            # a second step: the running statistics after two calls
        call()
        ref(dict(bd))
    torch.testing.assert_close(layer.norm.running_mean.double(), rl.norm.running_mean, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(layer.norm.running_var.double(), rl.norm.running_var, rtol=1e-6, atol=0)
    assert int(layer.norm.num_batches_tracked) == int(rl.norm.num_batches_tracked) == 2


# seeds for which the float64 preconditions hold (the first of base, base + 1000, ... that passes them; no case was changed for it)
PFN_SEEDS = dict(zip(PFN_SWEEP, (1100, 101, 5102, 103, 104, 1105, 106, 107, 108, 109, 110, 1111, 1112)))
PFN_VARIANT_SEEDS = dict(zip(PFN_VARIANTS, (200, 5201, 2202, 1203, 204, 205, 4206, 207, 208)))


@pytest.mark.parametrize("cfg", PFN_SWEEP, ids=lambda c: "C{}_dist{}_P{}_cout{}_V{}".format(*c))
def test_pfn_train_sweep_matches_float64(cfg):
    _pfn_case(cfg, PFN_SEEDS[cfg])


@pytest.mark.parametrize("name", list(PFN_VARIANTS))
def test_pfn_train_variants_match_float64(name):
    cfg, kw = PFN_VARIANTS[name]
    _pfn_case(cfg, PFN_VARIANT_SEEDS[name], **kw)


def test_pfn_sweep_covers_every_axis_value():
    cfgs = PFN_SWEEP + [c for c, _ in PFN_VARIANTS.values()]
    assert {c[0] for c in PFN_SWEEP} == set(range(3, 9)) and {c[1] for c in PFN_SWEEP} == {0, 1}
    assert {c[2] for c in PFN_SWEEP} == {1, 2, 20, 33, 63, 64} and {c[3] for c in PFN_SWEEP} == {1, 3, 16, 32, 60, 64}
    assert {c[4] for c in PFN_SWEEP} == {1, 3, 255, 257, 4001}
    assert (8, 1, 64, 64) in {c[:4] for c in cfgs} and (3, 0, 1, 1) in {c[:4] for c in cfgs}


# ------------------------------------------------------------------ 1b. scatter backward
SC_B, SC_NX, SC_NY = 3, 37, 29                                        # odd nx and ny


@pytest.mark.parametrize("as_float", [False, True], ids=["i32", "f32"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("ch", [32, 64, 128])
def test_scatter_backward_is_an_index_gather(ch, channels_last, as_float):
    """bit for bit: rows inside the canvas get the canvas gradient at their cell; negative y, y == ny, x == nx, x == -1, b == batch,
    b == -1 and the rows past the device count get exactly zero (x == nx and x == -1 would alias a cell of a neighbouring row if
    only the flattened cell index were checked)"""
    g = torch.Generator(device="cpu").manual_seed(300 + ch)
    V = 500
    cells = torch.randperm(SC_B * SC_NX * SC_NY, generator=g)[:V]
    b, r = cells // (SC_NX * SC_NY), cells % (SC_NX * SC_NY)
    coords = torch.stack([b, torch.zeros_like(b), r // SC_NX, r % SC_NX], 1).to(torch.int32)
    outside = torch.tensor([[0, 0, -1, 5], [1, 0, 3, SC_NX], [SC_B, 0, 2, 2], [2, 0, SC_NY, 0], [1, 0, 7, -1], [-1, 0, 4, 4]],
                           dtype=torch.int32)
    where = [7, 100, 101, 250, 333, 499]                              # spread among the inside rows
    inside = torch.ones(V, dtype=torch.bool)
    for w, o in zip(where, outside):
        coords[w] = o
        inside[w] = False
    tail = 21
    coords = torch.cat([coords, torch.full((tail, 4), -7, dtype=torch.int32)]).to(DEV)
    inside = torch.cat([inside, torch.zeros(tail, dtype=torch.bool)]).to(DEV)
    nvd = torch.tensor([V], dtype=torch.int32, device=DEV)
    feats = torch.randn((V + tail, ch), generator=g).to(DEV).requires_grad_()
    kc = coords.float() if as_float else coords
    canvas = pillar_ops.pillar_scatter_train(feats, kc, SC_B, SC_NX, SC_NY, num_voxels_dev=nvd, channels_last=channels_last)
    c = coords[inside].long()
    want = torch.zeros((SC_B, ch, SC_NY, SC_NX), device=DEV)
    want[c[:, 0], :, c[:, 2], c[:, 3]] = feats.detach()[inside]
    assert torch.equal(canvas, want)                                 # the forward leaves the outside pillars out too
    G = torch.randn((SC_B, ch, SC_NY, SC_NX), generator=g).to(DEV)
    G = G.contiguous(memory_format=torch.channels_last) if channels_last else G
    (canvas * G).sum().backward()
    ref = torch.zeros((V + tail, ch), device=DEV)
    ref[inside] = G[c[:, 0], :, c[:, 2], c[:, 3]]
    assert torch.equal(feats.grad.view(torch.int32), ref.view(torch.int32))
    assert bool((feats.grad[~inside] == 0).all())


# ------------------------------------------------------------------ 2. BatchNorm2d + ReLU train, the raw entry points
def _bn_params(ctot, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    gamma = torch.empty(ctot).uniform_(0.5, 1.5, generator=g)
    gamma[::3] *= -1.0
    return gamma, torch.empty(ctot).uniform_(-0.5, 0.5, generator=g)


def _bn_data(segs, rows, seed, quantised=False):
    """CPU: one (rows, ld) buffer per segment (C, ld, off).  quantised: z on a grid of 17 values per channel, so that however many
    rows there are a channel has 17 distinct pre-activations (a continuous z puts ~1e-5 of its elements within 1e-5 of the edge)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = []
    for _, ld, _ in segs:
        if quantised:
            xs.append(torch.randint(-8, 9, (rows, ld), generator=g).float() * 0.25 + torch.rand((1, ld), generator=g))
        else:
            xs.append(torch.randn((rows, ld), generator=g) * 1.7 + 0.8)
    return xs


def bn_reference(xs, segs, gamma, beta, eps, G, g_off):
    """float64 F.batch_norm(training=True) + ReLU with autograd on each segment's slice -> dict of float64 results"""
    r = dict(y=[], dz=[], dg=[], db=[], mean=[], var=[], pre=[])
    c0 = 0
    for x, (C_, ld, off) in zip(xs, segs):
        z = x[:, off:off + C_].double().requires_grad_()
        gm, bt = gamma[c0:c0 + C_].double().requires_grad_(), beta[c0:c0 + C_].double().requires_grad_()
        if eps > 0:
            pre = F.batch_norm(z, None, None, gm, bt, True, 0.0, eps)
        else:                                                        # F.batch_norm refuses eps == 0: the same formula, written out
            pre = (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False)) * gm + bt
        y = torch.relu(pre)
        (y * G[:, g_off + c0:g_off + c0 + C_].double()).sum().backward()
        for k, v in (("y", y.detach()), ("dz", z.grad), ("dg", gm.grad), ("db", bt.grad), ("mean", z.detach().mean(0)),
                     ("var", z.detach().var(0, unbiased=False)), ("pre", pre.detach())):
            r[k].append(v)
        c0 += C_
    return {k: (v if k == "dz" else torch.cat(v, -1)) for k, v in r.items()}


def bn_run(xs, segs, gamma, beta, eps, y_ld, y_off, G, g_off, ws_fill=None):
    """the raw C ABI on device buffers: -> (y buffer, [dx buffers], d_gamma, d_beta, batch_stats); y and every dx pre-filled with
    SENTINEL"""
    L = _lib.lib()
    n, rows = len(segs), xs[0].shape[0]
    ctot = sum(s[0] for s in segs)
    dev = xs[0].device
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    lds, offs, cs = (_lib.host_i32([s[i] for s in segs]) for i in (1, 2, 0))
    y = torch.full((rows, y_ld), SENTINEL, device=dev)
    stats = torch.empty(2 * ctot, dtype=torch.float64, device=dev)
    ss = torch.empty(2 * ctot, device=dev)
    bstats = torch.empty(3 * ctot, device=dev)
    wsb = L.lidar_bn_relu_train_workspace_bytes(rows, ctot)
    ws = torch.empty(wsb // 4, device=dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _lib.check(L.lidar_bn_relu_train_forward(n, ptrs, lds, offs, cs, rows, _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(y), y_ld,
                                             y_off, _lib.ptr(stats), _lib.ptr(ss), _lib.ptr(bstats), _lib.ptr(ws), wsb, _lib.stream()),
               "lidar_bn_relu_train_forward")
    dxs = [torch.full_like(x, SENTINEL) for x in xs]
    dptrs = (C.c_void_p * n)(*[d.data_ptr() for d in dxs])
    dg, db = torch.empty(ctot, device=dev), torch.empty(ctot, device=dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _lib.check(L.lidar_bn_relu_train_backward(n, ptrs, lds, offs, cs, rows, _lib.ptr(G), G.shape[1], g_off, _lib.ptr(gamma),
                                              _lib.ptr(stats), _lib.ptr(ss), dptrs, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(ws), wsb,
                                              _lib.stream()), "lidar_bn_relu_train_backward")
    return y, dxs, dg, db, bstats


def _bn_check(segs, rows, seed, y_pad=(0, 0), g_pad=(0, 0), eps=1e-3, quantised=False, plant=None, dev=None, check_only=False,
              exempt=()):
    """one call against float64.  y_pad / g_pad = (offset, slack): the output / gradient map is offset + ctot + slack floats wide.
    plant(xs, gamma, beta): edit the CPU inputs (special channels).  exempt: channels of the concatenated space left out of the
    1e-5 bars (the caller checks them its own way).  -> (kernel results, reference) for further checks"""
    dev = DEV if dev is None else dev
    ctot = sum(s[0] for s in segs)
    xs = _bn_data(segs, rows, seed, quantised)
    gamma, beta = _bn_params(ctot, seed + 1)
    if plant:
        plant(xs, gamma, beta)
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    y_off, y_ld = y_pad[0], y_pad[0] + ctot + y_pad[1]
    g_off, g_ld = g_pad[0], g_pad[0] + ctot + g_pad[1]
    G = torch.randn((rows, g_ld), generator=g)
    xs, gamma, beta, G = [x.to(dev) for x in xs], gamma.to(dev), beta.to(dev), G.to(dev)
    ref = bn_reference(xs, segs, gamma, beta, eps, G, g_off)
    keep = torch.ones(ctot, dtype=torch.bool, device=dev)
    for c in exempt:
        keep[c] = False
    edge = float(ref["pre"][:, keep].abs().min())
    print(f"bn {segs} rows {rows}: min |pre-activation| {edge:.3e}")
    assert edge > 1e-5
    if check_only:
        return None, ref
    y, dxs, dg, db, bstats = bn_run(xs, segs, gamma, beta, eps, y_ld, y_off, G, g_off)
    yk = y[:, y_off:y_off + ctot]
    errs = dict(y=rel(yk[:, keep], ref["y"][:, keep]), dg=rel(dg[keep], ref["dg"][keep]), db=rel(db[keep], ref["db"][keep]))
    assert bool((y[:, :y_off] == SENTINEL).all()) and bool((y[:, y_off + ctot:] == SENTINEL).all())
    c0, dz_err = 0, 0.0
    for dx, want, (C_, ld, off) in zip(dxs, ref["dz"], segs):
        k = keep[c0:c0 + C_]
        dz_err = max(dz_err, rel(dx[:, off:off + C_][:, k], want[:, k]) if bool(k.any()) else 0.0)
        assert bool((dx[:, :off] == SENTINEL).all()) and bool((dx[:, off + C_:] == SENTINEL).all())
        c0 += C_
    errs["dz"] = dz_err
    n = float(rows)
    mean, var, uvar = bstats[:ctot], bstats[ctot:2 * ctot], bstats[2 * ctot:]
    errs["mean"], errs["var"], errs["uvar"] = rel(mean, ref["mean"]), rel(var, ref["var"]), rel(uvar, ref["var"] * n / (n - 1))
    print(f"bn {segs} rows {rows}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(errs[k] < 1e-5 for k in ("y", "dz", "dg", "db")), errs
    assert all(errs[k] < 1e-6 for k in ("mean", "var", "uvar")), errs
    return dict(y=y, yk=yk, dxs=dxs, dg=dg, db=db, bstats=bstats, xs=xs, gamma=gamma, beta=beta, G=G, g_off=g_off, y_off=y_off,
                y_ld=y_ld), ref


# (C, ld, off) per segment; offsets of exactly 4 floats (16-byte alignment and no more), ld > off + C by different amounts
BN_WIDTHS = {
    "c4": [(4, 12, 4)], "c12": [(12, 20, 4)], "c20": [(20, 36, 12)], "c96": [(96, 104, 4)], "c100": [(100, 128, 20)],
    "c1000": [(1000, 1012, 4)], "c1024": [(1024, 1032, 4)],
    "seg2_100_12": [(100, 108, 4), (12, 32, 8)],
    "seg3_20_1000_4": [(20, 24, 0), (1000, 1008, 4), (4, 16, 4)],
    "seg4_4_96_1024_12": [(4, 8, 4), (96, 128, 28), (1024, 1028, 4), (12, 12, 0)],
}


BN_SEEDS = {name: 410 + 3 * i for i, name in enumerate(BN_WIDTHS)}   # seeds for which the float64 precondition holds


@pytest.mark.parametrize("name", list(BN_WIDTHS))
def test_bn_relu_widths_offsets_and_sentinels(name):
    """every declared width class (Q = C / 4 dividing 256 or not), 1..4 unequal segments, non-zero x_off / y_off / g_off"""
    _bn_check(BN_WIDTHS[name], 37, BN_SEEDS[name], y_pad=(4, 8), g_pad=(12, 4))


@pytest.mark.parametrize("rows", [2, 3, 255, 256, 257, 262144 + 77])
def test_bn_relu_row_counts(rows):
    """rows 2 .. 262221 at C = 12 and 4 (R = 85 and 256 rows per block pass); the last exceeds BT_MAX_BLOCKS * 256: blocks stride"""
    _bn_check([(12, 16, 4), (4, 8, 4)], rows, 500 + rows % 97, y_pad=(4, 0), g_pad=(0, 4), quantised=rows > 1000)


def test_bn_relu_constant_and_clamped_channels():
    """a channel constant over the rows: variance exactly 0, 1 / sigma = 1 / sqrt(eps), a finite unbiased variance; a channel whose
    y is <= 0 everywhere: d_gamma, d_beta and dz exactly 0"""
    eps = 1e-3

    def plant(xs, gamma, beta):
        xs[0][:, 4 + 5] = 2.5                                        # channel 5 of segment 0 (x_off 4): constant
        gamma[5], beta[5] = 0.75, 0.3
        gamma[9], beta[9] = 0.5, -40.0                               # channel 9: pre-activation < 0 everywhere
        gamma[14], beta[14] = -0.5, -40.0

    segs = [(12, 20, 4), (8, 8, 0)]
    out, ref = _bn_check(segs, 301, 611, y_pad=(8, 4), g_pad=(4, 0), eps=eps, plant=plant)
    var, uvar = out["bstats"][20:40], out["bstats"][40:60]
    assert float(var[5]) == 0.0 and float(uvar[5]) == 0.0 and bool(torch.isfinite(out["bstats"]).all())
    want = max(0.75 * 0.0 + 0.3, 0.0)                                # y = beta: z - mu is exactly 0 in float64
    assert float((out["yk"][:, 5] - want).abs().max()) < 1e-5
    # dz of the constant channel: gamma / sqrt(eps) (delta - mean delta), the z-hat term vanishing
    g5 = out["G"][:, out["g_off"] + 5].double()
    dz5 = 0.75 / eps ** 0.5 * (g5 - g5.mean())
    assert rel(out["dxs"][0][:, 4 + 5], dz5) < 1e-5
    for c, (seg, col) in ((9, (0, 4 + 9)), (14, (1, 2))):
        assert bool((out["yk"][:, c] == 0).all())
        assert float(out["dg"][c]) == 0.0 and float(out["db"][c]) == 0.0
        assert bool((out["dxs"][seg][:, col] == 0).all())


def test_bn_relu_eps_zero():
    _bn_check([(20, 24, 4), (4, 4, 0)], 129, 620, y_pad=(0, 4), g_pad=(4, 4), eps=0.0)


def test_bn_relu_nan_workspace_is_bitwise_the_same():
    segs = BN_WIDTHS["seg4_4_96_1024_12"]
    ctot = sum(s[0] for s in segs)
    xs = [x.to(DEV) for x in _bn_data(segs, 53, 630)]
    gamma, beta = (t.to(DEV) for t in _bn_params(ctot, 631))
    G = torch.randn((53, ctot + 8), generator=torch.Generator(device="cpu").manual_seed(632)).to(DEV)
    a = bn_run(xs, segs, gamma, beta, 1e-3, ctot + 4, 4, G, 8, ws_fill=0.0)
    b = bn_run(xs, segs, gamma, beta, 1e-3, ctot + 4, 4, G, 8, ws_fill=float("nan"))
    flat = lambda r: [r[0]] + list(r[1]) + list(r[2:])               # noqa: E731
    for u, v in zip(flat(a), flat(b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_bn_relu_large_mean_channel_within_4x_of_stock_fp32():
    """a channel with |mean| / sigma = 1e3 (z = 1250 + k / 4 on 17 grid values, so that no pre-activation lies within 1e-3 of the
    ReLU edge; the precondition is widened to the forward's error, below).  The backward takes mu, 1 / sigma and its sums from
    float64 and evaluates dz in float64, so dz, d_gamma and d_beta of this channel keep the ordinary 1e-5 bar.  The forward cannot:
    y = fma(z, scale, shift) in float32 has z * scale and shift of size |mean| / sigma ~ 1e3 each, one float32 rounding of either is
    up to 2^-24 * 1e3 = 6e-5 of the output's scale.  y is held to 4x the error of torch's own float32 BatchNorm2d + ReLU on the same
    input, floor 1e-5.  The other channels keep the 1e-5 bars.
    Measured on an MI355X, max |. - float64| / max |float64| over the channel, kernel / stock float32 (printed by the test):
        y 1.60e-05 / 1.95e-02;  dz 3.67e-08 / 2.10e-02;  d_gamma 1.38e-08 / 2.10e-02;  d_beta 2.32e-08 / 1.60e-07
    (with float32 dz coefficients and mu, as before this test existed: dz 6.06e-08, the rest the same)."""
    ch = 6

    def plant(xs, gamma, beta):
        g = torch.Generator(device="cpu").manual_seed(641)
        xs[0][:, 4 + ch] = 1250.0 + torch.randint(-8, 9, (xs[0].shape[0],), generator=g).float() * 0.25
        gamma[ch], beta[ch] = 1.1, 0.137

    segs = [(12, 20, 4)]
    out, ref = _bn_check(segs, 4096, 640, y_pad=(4, 4), g_pad=(4, 0), plant=plant, exempt=(ch,))
    assert float(ref["pre"][:, ch].abs().min()) > 1e-3
    assert 900 < abs(float(ref["mean"][ch])) / float(ref["var"][ch]) ** 0.5 < 1100
    # torch's float32 BatchNorm2d + ReLU, forward and backward, on the same input
    z = out["xs"][0][:, 4:16].clone().requires_grad_()
    gm, bt = out["gamma"].clone().requires_grad_(), out["beta"].clone().requires_grad_()
    ys = torch.relu(F.batch_norm(z.view(4096, 12, 1, 1), None, None, gm, bt, True, 0.0, 1e-3)).view(4096, 12)
    (ys * out["G"][:, 4:16]).sum().backward()
    pairs = dict(y=(out["yk"][:, ch], ys[:, ch], ref["y"][:, ch]), dz=(out["dxs"][0][:, 4 + ch], z.grad[:, ch], ref["dz"][0][:, ch]),
                 dg=(out["dg"][ch], gm.grad[ch], ref["dg"][ch]), db=(out["db"][ch], bt.grad[ch], ref["db"][ch]))
    res = {k: (rel(a, r), rel(s, r)) for k, (a, s, r) in pairs.items()}
    print("bn large-mean channel, kernel / stock fp32: " + "  ".join(f"{k} {a:.2e} / {s:.2e}" for k, (a, s) in res.items()))
    bad = {k: v for k, v in res.items() if not v[0] <= (max(4 * v[1], 1e-5) if k == "y" else 1e-5)}
    assert not bad, bad


# ------------------------------------------------------------------ 3. Winograd weight gradient, the raw entry point
def _wgrad_raw(B, H, W, cin, cout, x_ld, g_ld, x_off, g_off, seed, shift=0.3):
    """x = channels [x_off, x_off + cin) of a post-ReLU (B, H, W, x_ld) map, g = channels [g_off, ...) of a zero-mean (B, H, W, g_ld)
    one; dw pre-filled with NaN, the workspace too -> (dw, float64 reference)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    xb = torch.relu(torch.randn((B, H, W, x_ld), generator=gen) + shift).to(DEV)
    gb = torch.randn((B, H, W, g_ld), generator=gen).to(DEV)
    x, g = xb[..., x_off:x_off + cin].permute(0, 3, 1, 2), gb[..., g_off:g_off + cout].permute(0, 3, 1, 2)
    L = _lib.lib()
    wsb = L.lidar_wino43_wgrad_workspace_bytes(B, H, W, cin, cout)
    assert wsb > 0
    ws = torch.full((wsb // 4,), float("nan"), device=DEV)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    _lib.check(L.lidar_wino43_wgrad_nhwc(_lib.ptr(x), x_ld, _lib.ptr(g), g_ld, B, H, W, cin, cout, _lib.ptr(dw), _lib.ptr(ws), wsb,
                                         _lib.stream()), "lidar_wino43_wgrad_nhwc")
    assert bool(torch.isfinite(dw).all())                            # overwritten, not accumulated into
    return dw, _ref64(x, g)


@pytest.mark.parametrize("cin,cout", [(32, 512), (512, 32), (96, 160), (160, 96), (64, 128), (32, 32)])
def test_wgrad_rectangular_widths_and_unequal_strides(cin, cout):
    """Cin != Cout, x_ld != g_ld (both wider than their channel counts), slices that start 4 floats into a pixel (16 bytes)"""
    x_ld, g_ld = cin + 44, cout + 12
    assert x_ld != g_ld
    dw, ref = _wgrad_raw(2, 13, 10, cin, cout, x_ld, g_ld, 4, 4, 700 + cin)
    err = rel(dw, ref)
    print(f"wgrad43 raw cin {cin} cout {cout} x_ld {x_ld} g_ld {g_ld}: {err:.3e}")
    assert err <= BAR


def test_wgrad_every_small_map():
    """every (H, W) in 1..9 x 1..9 at (Cin, Cout) = (32, 64): partial tiles on both edges, maps smaller than one tile"""
    worst = 0.0
    for H in range(1, 10):
        for W in range(1, 10):
            dw, ref = _wgrad_raw(2, H, W, 32, 64, 36, 72, 4, 8, 800 + 10 * H + W)
            err = rel(dw, ref)
            print(f"wgrad43 raw map {H}x{W}: {err:.3e}")
            worst = max(worst, err)
            assert err <= BAR, (H, W, err)
    print(f"wgrad43 raw small maps, worst: {worst:.3e}")


# B * ceil(H / 4) * ceil(W / 4) tiles; at (512, 512) the split count is ceil(tiles / 512), so 512 | 513 and 1024 | 1025 cross it
WGRAD_TILES = {511: (7, 290, 4), 512: (2, 64, 64), 513: (1, 107, 74), 1025: (1, 100, 161)}


@pytest.mark.parametrize("cin,cout", [(512, 512), (32, 32)], ids=["c512", "c32"])
@pytest.mark.parametrize("tiles", list(WGRAD_TILES))
def test_wgrad_tile_counts_across_the_split(tiles, cin, cout):
    B, H, W = WGRAD_TILES[tiles]
    assert B * ((H + 3) // 4) * ((W + 3) // 4) == tiles
    dw, ref = _wgrad_raw(B, H, W, cin, cout, cin + 4, cout + 8, 4, 0, 900 + tiles)
    err = rel(dw, ref)
    print(f"wgrad43 raw {tiles} tiles (B, H, W) = {(B, H, W)} cin {cin} cout {cout}: {err:.3e}")
    assert err <= BAR


def test_wgrad_large_positive_mean_input():
    """post-ReLU x with mean / sigma = 8 against zero-mean g: the input transform's rows cancel the mean except one (row sums of
    B^T: 0, -6, 0, 0, 0, 0), whose position then carries 36 * mean into the fp32 accumulation"""
    dw, ref = _wgrad_raw(2, 30, 26, 64, 128, 64 + 8, 128 + 4, 4, 4, 950, shift=8.0)
    err = rel(dw, ref)
    print(f"wgrad43 raw large-mean x: {err:.3e}")
    assert err <= BAR
