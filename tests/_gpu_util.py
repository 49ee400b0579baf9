"""What the GPU test files share: the relative error, the end-of-module memory release, the PointPillar training inputs, the
config-dict conversion and the guard against host synchronisation.  A plain module (the test files import from it by name), no
conftest: nothing here changes how a test is collected or run."""
import contextlib
import gc

import numpy as np
import pytest
import torch

from lidardetection_amd.pcdet.utils.cfg import AttrDict


def rel(a, b, empty_ok=False):
    """max |a - b| / max(max |b|, 1e-30) in float64.  Tensors on different devices are compared on the host.  An empty `b` raises
    (an empty comparison is a bug of the test) unless empty_ok, where it is 0.0."""
    a, b = a.detach().double(), b.detach().double()
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    if empty_ok and b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def release(*workspaces):
    """hands the cached blocks (and the named lidardetection_amd workspaces) back to the device"""
    gc.collect()
    torch.cuda.synchronize()
    if workspaces:
        from lidardetection_amd import workspace
        for name in workspaces:
            workspace.drop(name)
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True, scope="module")
def release_memory():
    """the float64 comparisons hold tens of GB: hand the cached blocks back at the end of the module, so that later test files
    start from the same allocator state as without this one"""
    yield
    release()


def pp_inputs(B, seed, base):
    """-> points, offsets and (B, 12, 8) gt boxes (8 per frame) of B ring clouds synth.cloud_ring(base + seed + i), on cuda:0"""
    from lidardetection_amd import synth
    dev = torch.device("cuda:0")
    frames = [synth.cloud_ring(base + seed + i) for i in range(B)]
    pts = torch.from_numpy(np.concatenate(frames)).to(dev)
    offs = torch.tensor(np.cumsum([0] + [len(f) for f in frames]), dtype=torch.int32, device=dev)
    r = np.random.default_rng(seed)
    gt = np.zeros((B, 12, 8), np.float32)
    for b in range(B):
        n = 8
        gt[b, :n, 0] = r.uniform(5, 60, n)
        gt[b, :n, 1] = r.uniform(-30, 30, n)
        gt[b, :n, 2] = r.uniform(-1.5, -0.5, n)
        cls = r.integers(1, 4, n)
        size = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)[cls - 1]
        gt[b, :n, 3:6] = size * r.uniform(0.9, 1.1, (n, 1))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7] = cls
    return pts, offs, torch.from_numpy(gt).to(dev)


def to_cfg(d):
    return AttrDict({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


@contextlib.contextmanager
def no_host_sync(on=True):
    """inside: any host synchronisation raises (torch's sync-debug mode "error"); the previous mode comes back on every way out.
    on=False: no guard (for loops that guard only some iterations)."""
    prev = torch.cuda.get_sync_debug_mode()
    if on:
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(prev)
