"""The optimiser step of the reference's `adam_onecycle` training loop in three launches (csrc/optim_step.hip).

The reference does, after loss.backward() (tools/train_utils/train_utils.py:36-42):
    clip_grad_norm_(model.parameters(), GRAD_NORM_CLIP); optimizer.step()
where optimizer.step() is fastai's OptimWrapper.step (tools/train_utils/optimization/fastai_optim.py:132-149): a Python loop of
p.data.mul_(1 - wd * lr) over every parameter with requires_grad, then torch.optim.Adam.step() with betas (mom, 0.99).

AdamOneCycle.step() does the three with lidar_optim_grad_norm + lidar_optim_adam_step over a device-resident table of every
tensor's addresses: no per-tensor launch, no host synchronisation, bitwise reproducible.  There is no fall-back: a parameter the
kernels do not take (not float32, not contiguous, not on the GPU, sparse gradient) is refused with LidarHipError.
"""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from ._lib import LIMITS, LidarHipError

CHUNK, _ENTRY, WRITE_CLIPPED, ZERO_GRAD = (LIMITS["LIDAR_OPTIM_" + k] for k in ("CHUNK", "ENTRY", "WRITE_CLIPPED", "ZERO_GRAD"))
_BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def one_cycle(step, total_steps, lr_max=3e-3, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4):
    """-> (lr, mom) of the one-cycle schedule at `step` (what OneCycle.step(step) of
    tools/train_utils/optimization/learning_schedules_fastai.py:44-77 assigns to optimizer.lr / optimizer.mom), in host doubles.
    Two half-cosine phases meet at int(pct_start * total_steps): lr rises lr_max / div_factor -> lr_max while the momentum falls
    moms[0] -> moms[1], then lr falls to lr_max / div_factor / 1e4 while the momentum returns.  Every phase whose start is <= step
    is evaluated in order and the last one wins, so the first phase's formula never shows at or after the boundary."""
    def half_cos(a, b, frac):
        return b + (a - b) / 2 * (math.cos(math.pi * frac) + 1)

    low = lr_max / div_factor
    split = int(pct_start * total_steps)
    phases = [(0, split, (low, lr_max), (moms[0], moms[1])), (split, total_steps, (lr_max, low / 1e4), (moms[1], moms[0]))]
    lr = mom = None
    for start, end, lrs, ms in phases:
        if step >= start and end != start:
            frac = (step - start) / (end - start)
            lr, mom = half_cos(*lrs, frac), half_cos(*ms, frac)
    return lr, mom


def plan(numels):
    """lidar_optim_plan on the host: -> (chunk_tensor, chunk_index) int32 CPU tensors of the chunk map of a list of numel values"""
    L = _lib.lib()
    n = len(numels)
    arr = (C.c_longlong * max(n, 1))(*[int(v) for v in numels])
    total = L.lidar_optim_plan(arr, n, None, None, 0)
    if total < 0:
        raise LidarHipError(f"lidar_optim_plan failed with status {total}")
    ct, ci = torch.empty(total, dtype=torch.int32), torch.empty(total, dtype=torch.int32)
    if total:
        got = L.lidar_optim_plan(arr, n, C.c_void_p(ct.data_ptr()), C.c_void_p(ci.data_ptr()), total)
        assert got == total
    return ct, ci


def _leaf_modules(m):
    kids = list(m.children())
    return sum((_leaf_modules(k) for k in kids), []) if kids else [m]


def _module_params(module):
    """the reference's parameter order (optimization/__init__.py:20-32 with fastai_optim.split_bn_bias): the trainable parameters
    of the leaf modules that are not BatchNorm, then those of the BatchNorm leaves -> (params, group sizes)"""
    leaves = _leaf_modules(module)
    groups, seen = [], set()
    for want_bn in (False, True):
        ps = []
        for leaf in leaves:
            if isinstance(leaf, _BN_TYPES) == want_bn:
                for p in leaf.parameters():
                    if p.requires_grad and id(p) not in seen:
                        seen.add(id(p))
                        ps.append(p)
        groups.append(ps)
    return groups[0] + groups[1], [len(groups[0]), len(groups[1])]


class AdamOneCycle:
    """Adam with decoupled weight decay, gradient-norm clipping and a settable momentum: the optimiser build_optimizer returns for
    OPTIMIZER: adam_onecycle, with the loop's clip_grad_norm_ folded into step().  `lr` and `mom` are plain settable properties:
    the reference's OneCycle scheduler (or one_cycle() above) drives it unchanged.

    params_or_module: an nn.Module (the trainable parameters of its leaf modules, in the reference's order) or a list of parameters.
    state_dict() / load_state_dict() use torch.optim.Adam's layout."""

    def __init__(self, params_or_module, lr=3e-3, wd=0.01, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=10.0, amsgrad=False,
                 maximize=False):
        if amsgrad or maximize:
            raise LidarHipError("AdamOneCycle: amsgrad / maximize are not implemented by the fused step")
        if isinstance(params_or_module, nn.Module):
            self.params, self._group_sizes = _module_params(params_or_module)
        else:
            self.params = list(params_or_module)
            self._group_sizes = [len(self.params)]
        if len({id(p) for p in self.params}) != len(self.params):
            raise LidarHipError("AdamOneCycle: a parameter is listed twice")
        for i, p in enumerate(self.params):
            if not torch.is_tensor(p):
                raise LidarHipError(f"AdamOneCycle: parameter {i} is not a tensor")
            if p.dtype != torch.float32:
                raise LidarHipError(f"AdamOneCycle: parameter {i} is {p.dtype}; the fused step is float32 only")
            if not _dense(p):
                raise LidarHipError(f"AdamOneCycle: parameter {i} (shape {tuple(p.shape)}, strides {p.stride()}) is not contiguous "
                                    "(row-major or channels-last)")
            _check_grad(i, p, p.grad)
        devices = {p.device for p in self.params}
        if len(devices) > 1:
            raise LidarHipError(f"AdamOneCycle: parameters on more than one device ({sorted(str(d) for d in devices)})")
        if devices and next(iter(devices)).type != "cuda":
            raise LidarHipError("AdamOneCycle: expected CUDA (ROCm) parameters; this library has no CPU path")
        self.device = next(iter(devices)) if devices else None
        self._lr, self._mom, self.beta2, self.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        self.wd, self.max_grad_norm = float(wd), float(max_grad_norm)
        self._steps = [0] * len(self.params)    # per tensor, as torch keeps state['step']
        self._t = 0                             # steps of the optimiser itself
        self._sig = None
        if self.device is None:
            return
        # state: one flat buffer per moment, every tensor's slice 16-byte aligned
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        with torch.cuda.device(self.device):
            self._m_flat = torch.zeros(max(total, 4), dtype=torch.float32, device=self.device)
            self._v_flat = torch.zeros(max(total, 4), dtype=torch.float32, device=self.device)
            # the update is element-wise over memory: the moments take the parameter's (dense) strides
            self.exp_avg = [self._m_flat[o:o + p.numel()].as_strided(p.shape, p.stride()) for o, p in zip(offs, self.params)]
            self.exp_avg_sq = [self._v_flat[o:o + p.numel()].as_strided(p.shape, p.stride()) for o, p in zip(offs, self.params)]
            nt = len(self.params)
            self._max_chunks = sum((p.numel() + CHUNK - 1) // CHUNK for p in self.params)
            # device blob of 64-bit words: the table (nt entries), chunk_tensor (int32), chunk_index (int32)
            self._blob_words = nt * _ENTRY + self._max_chunks + 2
            self._blob = torch.zeros(self._blob_words, dtype=torch.int64, device=self.device)
            self._ct_off = nt * _ENTRY * 8
            self._ci_off = self._ct_off + (self._max_chunks * 4 + 7) // 8 * 8
            ws = _lib.lib().lidar_optim_workspace_bytes(max(self._max_chunks, 1))
            self._ws = torch.empty(ws // 8, dtype=torch.float64, device=self.device)
        self._n_active = self._n_chunks = 0

    # ---- hyper-parameters the schedulers assign
    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = float(value)

    @property
    def mom(self):
        return self._mom

    @mom.setter
    def mom(self, value):
        self._mom = float(value)

    @property
    def param_groups(self):
        groups, at = [], 0
        for n in self._group_sizes:
            groups.append({**self._group_defaults(), "params": self.params[at:at + n]})
            at += n
        return groups

    def _group_defaults(self):
        return {"lr": self._lr, "betas": (self._mom, self.beta2), "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": False}

    # ---- the device table
    def _active(self):
        """-> (signature, [(index, param, grad or None)]) of the parameters this step touches.  The signature holds what the device
        table holds: addresses and step lags."""
        sig, act = [], []
        for i, p in enumerate(self.params):
            if not p.requires_grad:
                continue
            g = p.grad
            if g is None:
                sig.append((p.data_ptr(), 0, 0))
            else:
                sig.append((p.data_ptr(), g.data_ptr(), self._t - self._steps[i]))
            act.append((i, p, g))
        return tuple(sig), act

    def _upload(self, sig, act):
        """rebuild table and chunk map in a pinned host buffer and copy them over on the current stream (the pinned allocator keeps
        the buffer alive until the copy has run)"""
        L = _lib.lib()
        for i, p, g in act:
            if p.device != self.device or p.dtype != torch.float32 or not _same_layout(p, self.exp_avg[i]):
                raise LidarHipError(f"AdamOneCycle: parameter {i} changed dtype, device or layout")
            _check_grad(i, p, g)
        host = torch.empty(self._blob_words, dtype=torch.int64, pin_memory=True)
        view = host.numpy()
        rows = view[:len(act) * _ENTRY].reshape(len(act), _ENTRY)
        for r, ((i, p, g), s) in enumerate(zip(act, sig)):
            rows[r] = (s[0], s[1], self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), p.numel(), s[2])
        numel = (C.c_longlong * max(len(act), 1))(*[p.numel() for _, p, _ in act])
        base = host.data_ptr()
        n_chunks = L.lidar_optim_plan(numel, len(act), C.c_void_p(base + self._ct_off), C.c_void_p(base + self._ci_off),
                                      self._max_chunks)
        if n_chunks < 0 or n_chunks > self._max_chunks:
            raise LidarHipError(f"lidar_optim_plan failed ({n_chunks})")
        self._blob.copy_(host, non_blocking=True)
        self._sig, self._n_active, self._n_chunks = sig, len(act), n_chunks

    # ---- torch.optim.Optimizer's surface
    def step(self, zero_grad=False):
        """clip to max_grad_norm, decay by 1 - wd * lr, Adam.  -> the total gradient norm before clipping, a 0-d device tensor (as
        clip_grad_norm_ returns).  The gradients are left clipped (what clip_grad_norm_ does), or zeroed with zero_grad=True."""
        if self.device is None:
            raise LidarHipError("AdamOneCycle.step: no parameters")
        L = _lib.lib()
        sig, act = self._active()
        with torch.cuda.device(self.device):
            if sig != self._sig:
                self._upload(sig, act)
            s = _lib.stream()
            table = self._blob.data_ptr()
            ct, ci = C.c_void_p(table + self._ct_off), C.c_void_p(table + self._ci_off)
            norm = torch.empty(2, dtype=torch.float32, device=self.device)
            _lib.check(L.lidar_optim_grad_norm(C.c_void_p(table), self._n_active, ct, ci, self._n_chunks, self.max_grad_norm,
                                               _lib.ptr(norm), _lib.ptr(self._ws), self._ws.numel() * 8, s), "lidar_optim_grad_norm")
            if self._n_chunks:
                _lib.check(L.lidar_optim_adam_step(C.c_void_p(table), self._n_active, ct, ci, self._n_chunks, _lib.ptr(norm),
                                                   self._lr, self._mom, self.beta2, self.eps, 1 - self.wd * self._lr,
                                                   self._t + 1, ZERO_GRAD if zero_grad else WRITE_CLIPPED, s),
                           "lidar_optim_adam_step")
        self._t += 1
        for i, _, g in act:
            if g is not None:
                self._steps[i] += 1
        # the kernels wrote behind torch's back: the version counters are what the folded-weight caches of this package (and
        # autograd's saved-tensor checks) go by
        _bump_versions([p for _, p, _ in act] + [g for _, _, g in act if g is not None])
        return norm[0]

    def zero_grad(self, set_to_none=False):
        if set_to_none:
            for p in self.params:
                p.grad = None
            return
        grads = [p.grad for p in self.params if p.grad is not None]
        for g in grads:
            if g.grad_fn is not None:
                g.detach_()
            else:
                g.requires_grad_(False)
        if grads:
            torch._foreach_zero_(grads)

    def state_dict(self):
        state = {}
        for i, n in enumerate(self._steps):
            if n > 0:
                state[i] = {"step": torch.tensor(float(n)), "exp_avg": self.exp_avg[i].clone(),
                            "exp_avg_sq": self.exp_avg_sq[i].clone()}
        groups, at = [], 0
        for n in self._group_sizes:
            groups.append({**self._group_defaults(), "params": list(range(at, at + n))})
            at += n
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(self.params):
            raise LidarHipError(f"AdamOneCycle.load_state_dict: {len(ids)} parameters in the state, {len(self.params)} here")
        if any(g.get("amsgrad") or g.get("maximize") for g in groups):
            raise LidarHipError("AdamOneCycle.load_state_dict: amsgrad / maximize are not implemented by the fused step")
        steps = []
        for k, pid in enumerate(ids):
            st = sd["state"].get(pid)
            if not st:
                steps.append(0)
                self.exp_avg[k].zero_()
                self.exp_avg_sq[k].zero_()
                continue
            for name, dst in (("exp_avg", self.exp_avg[k]), ("exp_avg_sq", self.exp_avg_sq[k])):
                src = st[name]
                if tuple(src.shape) != tuple(dst.shape):
                    raise LidarHipError(f"AdamOneCycle.load_state_dict: {name} of parameter {k} is {tuple(src.shape)}, "
                                        f"expected {tuple(dst.shape)}")
                dst.copy_(src)
            steps.append(int(float(st["step"])))
        self._steps, self._t, self._sig = steps, max(steps, default=0), None
        g0 = groups[0]
        self._lr, self.eps = float(g0["lr"]), float(g0.get("eps", self.eps))
        self._mom, self.beta2 = float(g0["betas"][0]), float(g0["betas"][1])


def _bump_versions(tensors):
    setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
    if setter is not None:
        try:
            setter(tensors, [t._version + 1 for t in tensors])
            return
        except TypeError:       # older torch: one tensor per call
            for t in tensors:
                setter(t, t._version + 1)
            return
    torch._foreach_mul_(tensors, 1.0)


def _check_grad(i, p, g):
    if g is None:
        return
    if g.is_sparse:
        raise LidarHipError(f"AdamOneCycle: parameter {i} has a sparse gradient")
    if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not _same_layout(g, p):
        raise LidarHipError(f"AdamOneCycle: the gradient of parameter {i} must be a float32 tensor of the parameter's shape and "
                            f"strides on its device, got {g.dtype} {tuple(g.shape)} strides {g.stride()} on {g.device}")


def _dense(p):
    """row-major, or channels-last (what PointPillarKITTI(channels_last=True) gives its convolution weights): the kernels walk memory"""
    return (p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))
            or (p.dim() == 5 and p.is_contiguous(memory_format=torch.channels_last_3d)))


def _same_layout(a, b):
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)
