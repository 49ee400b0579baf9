"""The fused optimiser step (lidardetection_amd/optim.py:AdamOneCycle, csrc/optim_step.hip) against the reference's own
optimizer and scheduler: tests/golden/optim_onecycle.npz holds six steps of build_optimizer / OneCycle / clip_grad_norm_ on
tests/_optim_model.py:Net in the reference's float32 and in float64 (tests/golden/make_optim_golden.py).

Bounds, per tensor and per step, against the float64 run:
  * total_norm within 2^-22 relative: the squares are exact in fp64, which leaves one fp32 rounding of the root;
  * parameters within 1e-4 of the tensor's scale (max |p|), the project's stated tolerance;
  * max |ours - fp64| <= max(4 x max |reference fp32 - fp64|, 2^-22 max |p|): a legitimately different fp32 operation order (FMA
    contraction, sqrt / divide forms) may cost a small multiple of the reference's own rounding, not more.
"""
import json
import os

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

from _gpu_util import no_host_sync
import _optim_model as om
from lidardetection_amd import optim, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 6


class Gold:
    def __init__(self, path):
        g = np.load(path)
        self.shapes = [tuple(s) for s in json.loads(str(g["shapes"]))]
        self.init, self.grads = om.split(g["init"], self.shapes), [om.split(a, self.shapes) for a in g["grads"]]
        self.lr, self.mom = g["lr"].tolist(), g["mom"].tolist()
        self.clip, self.wd = float(g["clip"]), float(g["wd"])
        self.norm32, self.norm64 = g["norm32"], g["norm64"]
        self.p32 = [om.split(a, self.shapes) for a in g["params32"]]
        self.p64 = [om.split(a, self.shapes) for a in g["params64"]]
        self.v64 = om.split(g["exp_avg_sq64"], self.shapes)
        self.m32, self.v32 = om.split(g["exp_avg32"], self.shapes), om.split(g["exp_avg_sq32"], self.shapes)

    def model(self, device=DEV):
        model = om.Net(device)
        params = om.reference_order(model)
        assert [tuple(p.shape) for p in params] == self.shapes
        with torch.no_grad():
            for p, a in zip(params, self.init):
                p.copy_(torch.from_numpy(a))
        return model, params

    def grad(self, it, device=DEV):
        return [torch.from_numpy(a.copy()).to(device) for a in self.grads[it]]     # a copy: the steps clip .grad in place

    def check_params(self, it, params, what=""):
        """the three parameter bounds of the module docstring at fixture step `it`"""
        for k, p in enumerate(params):
            ref64, ref32 = self.p64[it][k], self.p32[it][k].astype(np.float64)
            got = p.detach().cpu().numpy().astype(np.float64)
            scale = np.abs(ref64).max()
            dev, ref_dev = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
            assert dev <= 1e-4 * scale, (what, it, k, self.shapes[k], dev, scale)
            assert dev <= max(4 * ref_dev, 2.0 ** -22 * scale), (what, it, k, self.shapes[k], dev, ref_dev, scale)

    def check_norm(self, it, norm):
        assert abs(float(norm) - self.norm64[it]) <= 2.0 ** -22 * self.norm64[it], (it, float(norm), self.norm64[it])


@pytest.fixture(scope="module")
def gold(golden_dir):
    return Gold(os.path.join(golden_dir, "optim_onecycle.npz"))


def _replay(gold, steps=STEPS, fresh_buffers=False, check=False, **kw):
    """`steps` fused steps on the fixture's gradients and schedule -> (optimizer, params, [norm per step], [params per step])"""
    model, params = gold.model()
    opt = optim.AdamOneCycle(model, wd=gold.wd, max_grad_norm=gold.clip, **kw)
    assert all(a is b for a, b in zip(opt.params, params))
    norms, snaps, keep = [], [], []
    for it in range(steps):
        opt.lr, opt.mom = gold.lr[it], gold.mom[it]
        g = gold.grad(it)
        if fresh_buffers:
            keep.append([p.grad for p in params])           # the old buffers stay allocated: the new ones are elsewhere
            opt.zero_grad(set_to_none=True)
        if it == 0 or fresh_buffers:
            for p, a in zip(params, g):
                p.grad = a
        else:
            for p, a in zip(params, g):
                p.grad.copy_(a)
        norms.append(opt.step())
        snaps.append([p.detach().clone() for p in params])
        if check:
            gold.check_norm(it, norms[-1])
            gold.check_params(it, params)
    return opt, params, norms, snaps


@pytest.fixture(scope="module")
def base(gold):
    return _replay(gold)


def test_fixture_covers_the_shapes_and_the_eps_regime(gold):
    model, params = gold.model()
    sizes = [p.numel() for p in params]
    K = optim.CHUNK
    for n in (1, 3, 5, 7, K, K + 1, 3 * K + 2, 64, 16, 8 * 4 * 3 * 3):
        assert n in sizes
    assert sizes.count(8) >= 70
    off = params[om.offset_index(model)]
    assert off.numel() == 64 and off.data_ptr() % 16 == 4                       # 4-byte but not 16-byte aligned
    assert all(p.data_ptr() % 16 == 0 for k, p in enumerate(params) if k != om.offset_index(model))
    # the tiny-gradient tensor: sqrt(v) below 100 eps, so that eps in the denominator decides the update
    assert np.sqrt(gold.v64[om.tiny_index(model)]).max() < 100 * 1e-8
    assert (gold.norm64 < gold.clip).any() and (gold.norm64 > gold.clip).any()


def test_reference_replay(gold):
    opt, params, norms, _ = _replay(gold, check=True)
    assert all(n.is_cuda and n.dim() == 0 and n.dtype == torch.float32 for n in norms)
    # the final Adam state, at the same three bounds against the float64 state
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "optim_onecycle.npz"))
    for name, ours, ref32 in (("exp_avg64", opt.exp_avg, gold.m32), ("exp_avg_sq64", opt.exp_avg_sq, gold.v32)):
        for k, ref64 in enumerate(om.split(g[name], gold.shapes)):
            got = ours[k].cpu().numpy().astype(np.float64)
            scale = np.abs(ref64).max()
            dev, ref_dev = np.abs(got - ref64).max(), np.abs(ref32[k].astype(np.float64) - ref64).max()
            assert dev <= 1e-4 * scale and dev <= max(4 * ref_dev, 2.0 ** -22 * scale), (name, k, dev, ref_dev, scale)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(params))) and all(float(s["step"]) == STEPS for s in sd["state"].values())
    assert [len(gr["params"]) for gr in sd["param_groups"]] == [len(params) - 2 * om.N_BN, 2 * om.N_BN]
    assert all(p._version > 0 for p in params)          # the step is visible to version-keyed caches


def test_clip_boundary(gold):
    assert gold.norm64[0] < gold.clip < gold.norm64[1]
    _, _, _, clipped = _replay(gold, steps=1)
    model, params = gold.model()
    opt = optim.AdamOneCycle(model, wd=gold.wd, max_grad_norm=float("inf"))
    opt.lr, opt.mom = gold.lr[0], gold.mom[0]
    for p, a in zip(params, gold.grad(0)):
        p.grad = a
    opt.step()
    for a, b in zip(clipped[0], params):                   # below the threshold: the coefficient is exactly 1
        assert torch.equal(a, b.detach())
    for p, a in zip(params, gold.grad(0)):                 # ... and the gradients were written back unchanged
        assert torch.equal(p.grad, a)
    # above it: what step() leaves in .grad is grad * coef, coef = max_norm / (total_norm + 1e-6) in fp32
    model, params = gold.model()
    opt = optim.AdamOneCycle(model, wd=gold.wd, max_grad_norm=gold.clip)
    opt.lr, opt.mom = gold.lr[1], gold.mom[1]
    for p, a in zip(params, gold.grad(1)):
        p.grad = a
    norm = np.float32(opt.step().item())
    coef = np.float32(gold.clip) / (norm + np.float32(1e-6))
    assert coef.dtype == np.float32 and coef < 1
    for p, a in zip(params, gold.grad(1)):
        assert torch.equal(p.grad, a * float(coef))
    # zero_grad=True stores zeros instead
    for p, a in zip(params, gold.grad(2)):
        p.grad = a
    opt.step(zero_grad=True)
    assert all(not p.grad.any() for p in params)


def test_two_fresh_runs_are_bitwise_equal(gold, base):
    a, b = base, _replay(gold)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    for sa, sb in zip(a[3], b[3]):
        assert all(torch.equal(x, y) for x, y in zip(sa, sb))
    for name in ("exp_avg", "exp_avg_sq"):
        assert all(torch.equal(x, y) for x, y in zip(getattr(a[0], name), getattr(b[0], name)))
    assert a[0]._steps == b[0]._steps == [STEPS] * len(a[1])


def test_changing_gradient_buffers(gold, base):
    """zero_grad(set_to_none=True) between steps and new gradient tensors at new addresses: the table is uploaded again"""
    opt, params, norms, snaps = _replay(gold, fresh_buffers=True, check=True)
    for x, y in zip(norms, base[2]):
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(snaps[-1], base[3][-1]))


def _stock_step(params, adam, lr, mom, wd, clip):
    """one step the reference's way: clip_grad_norm_, OptimWrapper's decay loop, Adam with the scheduled betas"""
    norm = clip_grad_norm_(params, clip)
    for p in params:
        if p.requires_grad:
            p.data.mul_(1 - wd * lr)
    for g in adam.param_groups:
        g["lr"], g["betas"] = lr, (mom, 0.99)
    adam.step()
    return norm


def test_absent_and_frozen_parameters(gold):
    """grad None: decayed only, no state.  requires_grad False: untouched, outside the norm.  A parameter that sat out a step
    continues with its own step count (torch keeps `step` per parameter), checked against stock torch on the same device."""
    model, params = gold.model()
    ref_model, ref_params = gold.model()
    absent, frozen = 5, 2                                   # the chunk + 1 tensor, and the 5-element tail
    assert params[absent].numel() == optim.CHUNK + 1 and params[frozen].numel() == 5
    for ps in (params, ref_params):
        ps[frozen].requires_grad_(False)
    opt = optim.AdamOneCycle(params, wd=gold.wd, max_grad_norm=gold.clip)
    adam = torch.optim.Adam(ref_params, lr=0.0, betas=(0.9, 0.99))
    before = [p.detach().clone() for p in params]
    poison = torch.full_like(params[frozen], 1e6)
    for it in range(3):
        opt.lr, opt.mom = gold.lr[it], gold.mom[it]
        for ps in (params, ref_params):
            for k, (p, a) in enumerate(zip(ps, gold.grad(it))):
                p.grad = None if (k == absent and it == 0) else a
            ps[frozen].grad = poison.clone()                # a frozen parameter's gradient takes no part
        with_grad = [k for k in range(len(params)) if k != frozen and not (k == absent and it == 0)]
        exp_norm = np.sqrt(sum(float((gold.grads[it][k].astype(np.float64) ** 2).sum()) for k in with_grad))
        norm = opt.step()
        assert abs(float(norm) - exp_norm) <= 2.0 ** -22 * exp_norm
        assert torch.equal(params[frozen], before[frozen]) and torch.equal(params[frozen].grad, poison)
        if it == 0:
            assert torch.equal(params[absent].detach(), before[absent] * (1 - gold.wd * gold.lr[0]))
            assert params[absent].grad is None
            sd = opt.state_dict()["state"]
            assert absent not in sd and frozen not in sd and len(sd) == len(params) - 2
            assert not opt.exp_avg[absent].any() and not opt.exp_avg_sq[absent].any()
        ref_params[frozen].grad = None
        _stock_step(ref_params, adam, gold.lr[it], gold.mom[it], gold.wd, gold.clip)
        for k, (p, q) in enumerate(zip(params, ref_params)):
            scale = q.abs().max().item()
            assert (p - q).abs().max().item() <= 1e-4 * scale, (it, k)
    sd = opt.state_dict()["state"]
    assert float(sd[absent]["step"]) == 2 and float(sd[0]["step"]) == 3 and frozen not in sd


def test_state_interchange_with_torch_adam(gold):
    """three fused steps, then step 4 the reference's way on a stock torch.optim.Adam that loaded our state_dict (on the CPU: the
    reference's own arithmetic); and the reverse: three stock steps, our load_state_dict, a fused step 4"""
    opt, params, _, _ = _replay(gold, steps=3)
    sd = opt.state_dict()
    _, cpu_params = gold.model("cpu")
    with torch.no_grad():
        for q, p in zip(cpu_params, params):
            q.copy_(p.cpu())
    n_bn = 2 * om.N_BN
    adam = torch.optim.Adam([{"params": cpu_params[:-n_bn]}, {"params": cpu_params[-n_bn:]}], lr=0.0)
    adam.load_state_dict(sd)
    assert all(adam.state[q]["exp_avg"].device.type == "cpu" and float(adam.state[q]["step"]) == 3 for q in cpu_params)
    for q, a in zip(cpu_params, gold.grad(3, "cpu")):
        q.grad = a
    _stock_step(cpu_params, adam, gold.lr[3], gold.mom[3], gold.wd, gold.clip)
    gold.check_params(3, cpu_params, "ours -> stock")
    # our own fourth step from the same state, for completeness
    opt.lr, opt.mom = gold.lr[3], gold.mom[3]
    for p, a in zip(params, gold.grad(3)):
        p.grad.copy_(a)
    opt.step()
    gold.check_params(3, params, "ours")

    # reverse: the stock optimizer's three steps are the fixture's float32 run
    _, cpu_params = gold.model("cpu")
    adam = torch.optim.Adam([{"params": cpu_params[:-n_bn]}, {"params": cpu_params[-n_bn:]}], lr=0.0)
    for it in range(3):
        for q, a in zip(cpu_params, gold.grad(it, "cpu")):
            q.grad = a
        _stock_step(cpu_params, adam, gold.lr[it], gold.mom[it], gold.wd, gold.clip)
    model, params = gold.model()
    with torch.no_grad():
        for p, q in zip(params, cpu_params):
            p.copy_(q.to(DEV))
    opt = optim.AdamOneCycle(model, wd=gold.wd, max_grad_norm=gold.clip)
    opt.load_state_dict(adam.state_dict())
    assert opt._steps == [3] * len(params) and opt.lr == gold.lr[2] and opt.mom == gold.mom[2]
    opt.lr, opt.mom = gold.lr[3], gold.mom[3]
    for p, a in zip(params, gold.grad(3)):
        p.grad = a
    gold.check_norm(3, opt.step())
    gold.check_params(3, params, "stock -> ours")


def test_no_host_synchronisation(gold):
    model, params = gold.model()
    opt = optim.AdamOneCycle(model, wd=gold.wd, max_grad_norm=gold.clip)
    opt.lr, opt.mom = gold.lr[0], gold.mom[0]
    first, second = gold.grad(0), gold.grad(1)
    for p, a in zip(params, first):
        p.grad = a
    opt.step()                                              # warm-up: code objects, the first table upload
    torch.cuda.synchronize()
    with no_host_sync():
        opt.step()
        opt.zero_grad()
        opt.step(zero_grad=True)
        opt.zero_grad(set_to_none=True)
        for p, a in zip(params, second):                    # new addresses: the step re-uploads the table
            p.grad = a
        sig = opt._sig
        norm = opt.step()
        assert opt._sig != sig
        opt.zero_grad(set_to_none=True)
    assert torch.isfinite(norm).item() and all(p.grad is None for p in params)


def _pp_inputs(B, seed):
    frames = [synth.cloud_ring(2100 + seed + i) for i in range(B)]
    pts = torch.from_numpy(np.concatenate(frames)).to(DEV)
    offs = torch.tensor(np.cumsum([0] + [len(f) for f in frames]), dtype=torch.int32, device=DEV)
    r = np.random.default_rng(seed)
    gt = np.zeros((B, 12, 8), np.float32)
    size = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    for b in range(B):
        n = 8
        cls = r.integers(1, 4, n)
        gt[b, :n, 0], gt[b, :n, 1], gt[b, :n, 2] = r.uniform(5, 60, n), r.uniform(-30, 30, n), r.uniform(-1.5, -0.5, n)
        gt[b, :n, 3:6] = size[cls - 1] * r.uniform(0.9, 1.1, (n, 1))
        gt[b, :n, 6], gt[b, :n, 7] = r.uniform(-np.pi, np.pi, n), cls
    return pts, offs, torch.from_numpy(gt).to(DEV)


def test_train_step_end_to_end_matches_the_stock_tail():
    """three PointPillarKITTI.train_step()s against the same model stepped the stock way (train_loss + backward + clip_grad_norm_ +
    the decay loop + torch.optim.Adam), at batch 2 (the batch the other train-path tests of the class use).  Every loss term and
    the norm at 1e-4 relative, not bitwise.

    The library's convolution weight gradients run in their deterministic mode here (torch.backends.cudnn.deterministic).  Adam's
    update is m / (sqrt(v) + eps), close to lr * sign(g) in the first steps, so last-bit noise in a gradient near zero moves a weight
    by a whole lr: measured on an MI355X, two identical STOCK runs with the default (atomic) weight gradients are 2e-3 apart in the
    parameters after three steps and 6e-5 to 3e-4 apart in the third step's loc loss, which says nothing about the optimiser.
    With deterministic gradients two stock runs are bitwise equal, and what is left is the fused step's own rounding (3e-7 of a
    tensor's scale against the stock tail on the same gradients): 1.1e-5 in the third loc loss, 3.4e-6 in the third norm."""
    from lidardetection_amd.pointpillar import PointPillarKITTI
    pts, offs, gt = _pp_inputs(2, 17)
    models = []
    for _ in range(2):
        torch.manual_seed(4)
        models.append(PointPillarKITTI(batch_size=2, device=DEV).train())
    fused, stock = models
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _three_train_steps(fused, stock, pts, offs, gt)
    finally:
        torch.backends.cudnn.deterministic = was


def _three_train_steps(fused, stock, pts, offs, gt):
    opt = optim.AdamOneCycle(fused, wd=0.01, max_grad_norm=10.0)
    stock_params = [p for p in stock.parameters() if p.requires_grad]
    assert len(opt.params) == len(stock_params) and sum(p.numel() for p in opt.params) == sum(p.numel() for p in stock_params)
    adam = torch.optim.Adam(stock_params, lr=0.0, betas=(0.9, 0.99))
    for it in range(3):
        lr, mom = optim.one_cycle(it, 10)
        opt.lr, opt.mom = lr, mom
        with no_host_sync(it == 2):    # once everything is warm: no host synchronisation
            out = fused.train_step(pts, offs, gt, opt)
        assert len(out) == 4 and all(t.is_cuda and not t.requires_grad for t in out)
        adam.zero_grad()
        losses = stock.train_loss(pts, offs, gt)
        sum(losses).backward()
        norm = _stock_step(stock_params, adam, lr, mom, 0.01, 10.0)
        print("step", it, "fused", [float(a) for a in out], "stock", [float(b.detach()) for b in list(losses) + [norm]])
        for a, b in zip(out, list(losses) + [norm]):
            torch.testing.assert_close(a, b.detach(), rtol=1e-4, atol=1e-6)
