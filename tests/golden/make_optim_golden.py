"""Generates tests/golden/optim_onecycle.npz from the REFERENCE ITSELF: its own build_optimizer (OptimWrapper over torch.optim.Adam,
OPTIMIZER: adam_onecycle) and build_scheduler (OneCycle) of tools/train_utils/optimization, with torch's clip_grad_norm_, stepped
the way tools/train_utils/train_utils.py:25-42 steps them, on the CPU.  Runs only where the reference checkout is (default
/root/reference, or $LIDAR_REFERENCE); the .npz is what the tests read.

Shim: fastai_optim.py imports collections.Iterable, which current Python keeps in collections.abc; it is aliased before the import.

The model is tests/_optim_model.py:Net; no forward pass: every step assigns .grad from a seeded array.  The schedule is the
OPTIMIZATION block of tools/cfgs/kitti_models/pointpillar.yaml with total_steps = 10, so that six steps cross the PCT_START
boundary at step 4.  The gradient scale changes per step so that the total norm lies below GRAD_NORM_CLIP on some steps and above
it on others (asserted); the `tiny` tensor's gradients are of order 1e-8 throughout.

Two runs of the same six steps: the reference's own float32, and float64 (model.double(), the float32 gradients converted
exactly).  Stored, parameters concatenated flat in the optimizer's order (param_groups[0] then [1]): shapes (JSON), group_sizes,
init (N) f32, grads (6, N) f32, lr / mom (6) f64, clip, wd, total_steps, norm32 (6) f32, norm64 (6) f64, params32 (6, N) f32,
params64 (6, N) f64, the final Adam state exp_avg{32,64}, exp_avg_sq{32,64} and steps.

Usage:  python tests/golden/make_optim_golden.py
"""
import collections
import collections.abc
import json
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _optim_model as om  # noqa: E402

REF = os.environ.get("LIDAR_REFERENCE", "/root/reference")
STEPS, TOTAL_STEPS = 6, 10
GRAD_SCALE = [0.05, 0.3, 0.02, 0.6, 0.1, 1.0]


def reference_optimization():
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable
    sys.path.insert(0, os.path.join(REF, "tools"))
    from train_utils.optimization import build_optimizer, build_scheduler
    return build_optimizer, build_scheduler


def optim_cfg():
    with open(os.path.join(REF, "tools", "cfgs", "kitti_models", "pointpillar.yaml")) as fh:
        return types.SimpleNamespace(**yaml.safe_load(fh)["OPTIMIZATION"])


def run(dtype, init, grads, cfg):
    from torch.nn.utils import clip_grad_norm_
    build_optimizer, build_scheduler = reference_optimization()
    model = om.Net()
    order = om.reference_order(model)
    shapes = [tuple(p.shape) for p in order]
    with torch.no_grad():
        for p, a in zip(order, om.split(init, shapes)):
            p.copy_(torch.from_numpy(a))
    if dtype == torch.float64:
        model.double()
    opt = build_optimizer(model, cfg)
    params = [p for g in opt.param_groups for p in g["params"]]
    assert [tuple(p.shape) for p in params] == shapes
    assert all(a.dtype == dtype and torch.equal(a, b) for a, b in zip(params, om.reference_order(model)))
    sched, _ = build_scheduler(opt, total_iters_each_epoch=TOTAL_STEPS, total_epochs=1, last_epoch=-1, optim_cfg=cfg)
    out = {"lr": [], "mom": [], "norm": [], "params": []}
    for it in range(STEPS):
        sched.step(it)
        out["lr"].append(float(opt.lr))
        out["mom"].append(float(opt.mom))
        opt.zero_grad()
        for p, a in zip(params, om.split(grads[it], shapes)):
            p.grad = torch.from_numpy(a.copy()).to(dtype)
        out["norm"].append(clip_grad_norm_(model.parameters(), cfg.GRAD_NORM_CLIP).item())
        opt.step()
        out["params"].append(np.concatenate([p.detach().numpy().reshape(-1) for p in params]))
    st = opt.state_dict()["state"]
    out["exp_avg"] = np.concatenate([st[k]["exp_avg"].numpy().reshape(-1) for k in range(len(params))])
    out["exp_avg_sq"] = np.concatenate([st[k]["exp_avg_sq"].numpy().reshape(-1) for k in range(len(params))])
    out["steps"] = np.array([int(float(st[k]["step"])) for k in range(len(params))], np.int64)
    out["group_sizes"] = np.array([len(g["params"]) for g in opt.param_groups], np.int64)
    return out, shapes


def main():
    cfg = optim_cfg()
    assert cfg.OPTIMIZER == "adam_onecycle"
    model = om.Net()
    order = om.reference_order(model)
    shapes = [tuple(p.shape) for p in order]
    sizes = [p.numel() for p in order]
    n = sum(sizes)
    r = np.random.default_rng(20251019)
    init = (r.standard_normal(n) * 0.1).astype(np.float32)
    tiny, at = om.tiny_index(model), np.cumsum([0] + sizes)
    first_bn = len(order) - 2 * om.N_BN
    for k in range(first_bn, len(order), 2):          # BatchNorm weights (weight, bias alternate) near 1, as trained ones are
        init[at[k]:at[k + 1]] += 1.0
    grads = np.stack([(r.standard_normal(n) * s).astype(np.float32) for s in GRAD_SCALE])
    grads[:, at[tiny]:at[tiny + 1]] = (r.standard_normal((STEPS, sizes[tiny])) * om.TINY_GRAD).astype(np.float32)
    o32, s32 = run(torch.float32, init, grads, cfg)
    o64, s64 = run(torch.float64, init, grads, cfg)
    assert s32 == s64 == shapes and o32["lr"] == o64["lr"] and o32["mom"] == o64["mom"]
    below = [v < cfg.GRAD_NORM_CLIP for v in o64["norm"]]
    assert any(below) and not all(below), o64["norm"]
    assert min(abs(v - cfg.GRAD_NORM_CLIP) for v in o64["norm"]) > 0.5, o64["norm"]      # no step sits on the clip boundary
    assert TOTAL_STEPS * cfg.PCT_START < STEPS - 1
    out = os.path.join(HERE, "optim_onecycle.npz")
    np.savez_compressed(
        out, shapes=json.dumps([list(s) for s in shapes]), group_sizes=o32["group_sizes"], init=init, grads=grads,
        lr=np.array(o32["lr"], np.float64), mom=np.array(o32["mom"], np.float64), clip=np.float64(cfg.GRAD_NORM_CLIP),
        wd=np.float64(cfg.WEIGHT_DECAY), total_steps=np.int64(TOTAL_STEPS), lr_max=np.float64(cfg.LR),
        moms=np.array(cfg.MOMS, np.float64), div_factor=np.float64(cfg.DIV_FACTOR), pct_start=np.float64(cfg.PCT_START),
        norm32=np.array(o32["norm"], np.float32), norm64=np.array(o64["norm"], np.float64),
        params32=np.stack(o32["params"]).astype(np.float32), params64=np.stack(o64["params"]).astype(np.float64),
        exp_avg32=o32["exp_avg"].astype(np.float32), exp_avg_sq32=o32["exp_avg_sq"].astype(np.float32),
        exp_avg64=o64["exp_avg"].astype(np.float64), exp_avg_sq64=o64["exp_avg_sq"].astype(np.float64), steps=o32["steps"])
    print(out, os.path.getsize(out), "bytes; norms", o64["norm"], "lr", o32["lr"], "mom", o32["mom"])


if __name__ == "__main__":
    main()
