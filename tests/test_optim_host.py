"""Host-side checks of the fused optimiser step (lidardetection_amd/optim.py, csrc/optim_step.hip): the one-cycle schedule against
the reference's own OneCycle (tests/golden/optim_onecycle.npz, written by tests/golden/make_optim_golden.py), the pure-host chunk
plan, the refusals, and the state_dict layout against torch.optim.Adam.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import _optim_model as om
from lidardetection_amd import _lib, optim
from lidardetection_amd._lib import LidarHipError


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "optim_onecycle.npz"))


def test_one_cycle_equals_the_reference_schedule(gold):
    total = int(gold["total_steps"])
    args = (total, float(gold["lr_max"]), tuple(gold["moms"].tolist()), float(gold["div_factor"]), float(gold["pct_start"]))
    assert len(gold["lr"]) == 6 and int(float(gold["pct_start"]) * total) < 5      # the stored steps cross the phase boundary
    for step, (lr, mom) in enumerate(zip(gold["lr"], gold["mom"])):
        got_lr, got_mom = optim.one_cycle(step, *args)
        assert abs(got_lr - lr) <= 1e-12 * abs(lr), (step, got_lr, lr)
        assert abs(got_mom - mom) <= 1e-12 * abs(mom), (step, got_mom, mom)
    # at the boundary the second phase has overwritten the first: its start values, not the first phase's formula past its end
    lr, mom = optim.one_cycle(4, *args)
    assert abs(lr - args[1]) <= 1e-12 * args[1] and abs(mom - args[2][1]) <= 1e-12


def test_one_cycle_drives_like_the_reference_scheduler_object():
    """the reference's OneCycle only assigns optimizer.lr and optimizer.mom: both are plain settable properties"""
    with pytest.raises(LidarHipError):
        optim.AdamOneCycle([nn.Parameter(torch.zeros(3))])         # (CPU parameters are refused; the properties are on the class)
    assert isinstance(optim.AdamOneCycle.lr, property) and optim.AdamOneCycle.lr.fset is not None
    assert isinstance(optim.AdamOneCycle.mom, property) and optim.AdamOneCycle.mom.fset is not None


def _plan(numels):
    ct, ci = optim.plan(numels)
    return ct.tolist(), ci.tolist()


def test_plan_covers_every_element_once():
    K = optim.CHUNK
    L = _lib.lib()
    assert K == 1024
    numels = [1, 3, 5, 7, K, K + 1, 3 * K + 2, 64, 0, 8, 8, 288]
    ct, ci = _plan(numels)
    # chunk boundaries: tensor by tensor, ceil(numel / K) chunks each, indices ascending from 0; an empty tensor has none
    exp = [(t, i) for t, n in enumerate(numels) for i in range((n + K - 1) // K)]
    assert list(zip(ct, ci)) == exp
    assert [c for c in zip(ct, ci) if c[0] == 4] == [(4, 0)]                       # exactly one chunk
    assert [c for c in zip(ct, ci) if c[0] == 5] == [(5, 0), (5, 1)]               # one chunk + 1
    assert [c for c in zip(ct, ci) if c[0] == 6] == [(6, 0), (6, 1), (6, 2), (6, 3)]
    assert 8 not in ct
    cover = [np.zeros(n, np.int32) for n in numels]
    for t, i in zip(ct, ci):
        cover[t][i * K:min((i + 1) * K, numels[t])] += 1
    assert all((c == 1).all() for c in cover)
    # counting only, a capacity smaller than the plan, and bad arguments
    arr = (C.c_longlong * len(numels))(*numels)
    assert L.lidar_optim_plan(arr, len(numels), None, None, 0) == len(exp)
    few_t, few_i = (C.c_int * 4)(*[-7] * 4), (C.c_int * 4)(*[-7] * 4)
    assert L.lidar_optim_plan(arr, len(numels), few_t, few_i, 3) == len(exp)
    assert list(few_t) == [0, 1, 2, -7] and list(few_i) == [0, 0, 0, -7]
    assert L.lidar_optim_plan((C.c_longlong * 1)(-1), 1, None, None, 0) == -1
    assert L.lidar_optim_plan(None, 2, None, None, 0) == -1


def test_plan_of_an_empty_list_and_workspace_query():
    L = _lib.lib()
    assert _plan([]) == ([], [])
    assert L.lidar_optim_plan(None, 0, None, None, 0) == 0
    assert L.lidar_optim_workspace_bytes(0) == 0
    assert L.lidar_optim_workspace_bytes(5) >= 5 * 8
    # argument errors come back as a status before any launch
    assert L.lidar_optim_grad_norm(None, 1, None, None, 4, 10.0, None, None, 0, None) == -1
    assert L.lidar_optim_adam_step(None, 1, None, None, 4, None, 1e-3, 0.9, 0.99, 1e-8, 1.0, 1, 1, None) == -1


def test_refusals():
    ok = nn.Parameter(torch.zeros(4))
    with pytest.raises(LidarHipError, match="float32 only"):
        optim.AdamOneCycle([nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(LidarHipError, match="float32 only"):
        optim.AdamOneCycle([nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(LidarHipError, match="not contiguous"):
        optim.AdamOneCycle([nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(LidarHipError, match="not contiguous"):
        optim.AdamOneCycle([nn.Parameter(torch.zeros(8)[::2])])
    with pytest.raises(LidarHipError, match="no CPU path"):
        optim.AdamOneCycle([ok])
    with pytest.raises(LidarHipError, match="no CPU path"):
        optim.AdamOneCycle(nn.Linear(3, 2))
    sparse = nn.Parameter(torch.zeros(4, 2))
    sparse.grad = torch.sparse_coo_tensor(torch.tensor([[1], [0]]), torch.tensor([1.0]), (4, 2))
    with pytest.raises(LidarHipError, match="sparse gradient"):
        optim.AdamOneCycle([sparse])
    with pytest.raises(LidarHipError, match="more than one device"):
        optim.AdamOneCycle([ok, nn.Parameter(torch.zeros(4, device="meta"))])
    with pytest.raises(LidarHipError, match="amsgrad"):
        optim.AdamOneCycle([ok], amsgrad=True)
    with pytest.raises(LidarHipError, match="maximize"):
        optim.AdamOneCycle([ok], maximize=True)
    with pytest.raises(LidarHipError, match="listed twice"):
        optim.AdamOneCycle([ok, ok])


def test_module_parameters_come_in_the_reference_order(gold):
    """leaf modules flattened, the trainable parameters of the non-BatchNorm leaves first, then the BatchNorm ones
    (optimization/__init__.py:20-32, fastai_optim.split_bn_bias): the order the fixture's optimizer had"""
    model = om.Net()
    model.conv.weight.requires_grad_(True)
    params, sizes = optim._module_params(model)
    assert [list(p.shape) for p in params] == json.loads(str(gold["shapes"]))
    assert sizes == gold["group_sizes"].tolist() == [len(params) - 2 * om.N_BN, 2 * om.N_BN]
    assert all(a is b for a, b in zip(params, om.reference_order(model)))
    model.tails.p1.requires_grad_(False)                       # trainable_params filters at construction
    assert len(optim._module_params(model)[0]) == len(params) - 1


def _cpu_instance(params, steps):
    """an AdamOneCycle over CPU tensors, built past the device refusal: only the state_dict code runs on it"""
    o = object.__new__(optim.AdamOneCycle)
    o.params, o._group_sizes = list(params), [len(params)]
    o._lr, o._mom, o.beta2, o.eps, o.wd, o.max_grad_norm = 2e-3, 0.87, 0.99, 1e-8, 0.01, 10.0
    o._steps, o._t, o._sig = list(steps), max(steps), None
    g = torch.Generator().manual_seed(5)
    o.exp_avg = [torch.randn(p.shape, generator=g) for p in params]
    o.exp_avg_sq = [torch.rand(p.shape, generator=g) for p in params]
    return o


def test_state_dict_layout_loads_into_torch_adam_and_back():
    params = [nn.Parameter(torch.randn(s)) for s in ((5,), (2, 3), (4,))]
    ours = _cpu_instance(params, [3, 3, 0])                     # the last parameter never had a gradient: no state
    sd = ours.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1]
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert sd["param_groups"][0]["params"] == [0, 1, 2] and sd["param_groups"][0]["lr"] == 2e-3
    assert sd["param_groups"][0]["betas"] == (0.87, 0.99)
    stock = torch.optim.Adam(params, lr=1.0)
    stock.load_state_dict(sd)
    g = stock.param_groups[0]
    assert g["lr"] == 2e-3 and tuple(g["betas"]) == (0.87, 0.99) and g["weight_decay"] == 0 and not g["amsgrad"]
    for k in (0, 1):
        st = stock.state[params[k]]
        assert float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], ours.exp_avg[k]) and torch.equal(st["exp_avg_sq"], ours.exp_avg_sq[k])
    assert params[2] not in stock.state
    for p in params:
        p.grad = torch.ones_like(p)
    stock.step()                                                # a stock Adam continues from ours
    assert float(stock.state[params[0]]["step"]) == 4.0 and float(stock.state[params[2]]["step"]) == 1.0
    # ... and ours takes torch's state_dict (two groups, as the reference's optimizer has: the ids are taken in group order)
    back = _cpu_instance(params, [0, 0, 0])
    sd2 = stock.state_dict()
    sd2["param_groups"] = [dict(sd2["param_groups"][0], params=[0, 1]), dict(sd2["param_groups"][0], params=[2])]
    back.load_state_dict(sd2)
    assert back._steps == [4, 4, 1] and back._t == 4 and back.lr == 2e-3 and back.mom == 0.87 and back.beta2 == 0.99
    for k in range(3):
        assert torch.equal(back.exp_avg[k], stock.state[params[k]]["exp_avg"])
        assert torch.equal(back.exp_avg_sq[k], stock.state[params[k]]["exp_avg_sq"])
    with pytest.raises(LidarHipError):
        back.load_state_dict({"state": {}, "param_groups": [dict(sd2["param_groups"][0], params=[0])]})
    with pytest.raises(LidarHipError):
        back.load_state_dict({"state": {}, "param_groups": [dict(sd["param_groups"][0], amsgrad=True)]})
