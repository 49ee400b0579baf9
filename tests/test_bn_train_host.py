"""Host checks (no device) of lidardetection_amd/bn_train.py, the one copy of what the fused train-mode BatchNorm routes share: the
predicate over a table of modules, with the three wrappers' answers written out from what bev_train.bn_supported,
spconv.train.bn_supported and sa_train._bn_ok answered before they shared it, and the running-statistics update against
torch.nn.functional.batch_norm(training=True)'s own."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from lidardetection_amd import bev_train, bn_train, sa_train
from lidardetection_amd.spconv import train as sp_train

B1, B2 = nn.BatchNorm1d, nn.BatchNorm2d
T, N = True, False

# label: (module, channels argument,
#         supported(.., B2, False), supported(.., B2, True), supported(.., B1, True), supported(.., B2, True, max_c=None),
#         bev_train.bn_supported, spconv.train.bn_supported, sa_train._bn_ok (which takes the module alone))
TABLE = {
    "2d":               (lambda: B2(64), None,                                  T, T, N, T,  T, N, T),
    "1d":               (lambda: B1(64), None,                                  N, N, T, N,  N, T, N),
    "2d affine=False":  (lambda: B2(64, affine=False), None,                    N, N, N, N,  N, N, N),
    "1d affine=False":  (lambda: B1(64, affine=False), None,                    N, N, N, N,  N, N, N),
    "2d no running":    (lambda: B2(64, track_running_stats=False), None,       N, N, N, N,  N, N, N),
    "1d no running":    (lambda: B1(64, track_running_stats=False), None,       N, N, N, N,  N, N, N),
    "2d momentum=None": (lambda: B2(64, momentum=None), None,                   N, N, N, N,  N, N, N),
    "1d momentum=None": (lambda: B1(64, momentum=None), None,                   N, N, N, N,  N, N, N),
    "2d eval":          (lambda: B2(64).eval(), None,                           T, N, N, N,  T, N, N),
    "1d eval":          (lambda: B1(64).eval(), None,                           N, N, N, N,  N, N, N),
    "2d width 0":       (lambda: B2(0), None,                                   N, N, N, T,  N, N, T),
    "2d width 4":       (lambda: B2(4), None,                                   T, T, N, T,  T, N, T),
    "2d width 6":       (lambda: B2(6), None,                                   N, N, N, T,  N, N, T),
    "2d width 1024":    (lambda: B2(1024), None,                                T, T, N, T,  T, N, T),
    "2d width 1028":    (lambda: B2(1028), None,                                N, N, N, T,  N, N, T),
    "1d width 0":       (lambda: B1(0), None,                                   N, N, N, N,  N, N, N),
    "1d width 4":       (lambda: B1(4), None,                                   N, N, T, N,  N, T, N),
    "1d width 6":       (lambda: B1(6), None,                                   N, N, N, N,  N, N, N),
    "1d width 1024":    (lambda: B1(1024), None,                                N, N, T, N,  N, T, N),
    "1d width 1028":    (lambda: B1(1028), None,                                N, N, N, N,  N, N, N),
    "2d other width":   (lambda: B2(64), 32,                                    N, N, N, N,  N, N, T),
    "1d other width":   (lambda: B1(64), 32,                                    N, N, N, N,  N, N, N),
    "2d same width":    (lambda: B2(64), 64,                                    T, T, N, T,  T, N, T),
}


@pytest.mark.parametrize("label", list(TABLE))
def test_predicate_and_its_three_wrappers(label):
    make, ch, s2, s2t, s1t, s2t_any, bev, sp, sa = TABLE[label]
    bn = make()
    assert bn_train.supported(bn, B2, False, ch) is s2
    assert bn_train.supported(bn, B2, True, ch) is s2t
    assert bn_train.supported(bn, B1, True, ch) is s1t
    assert bn_train.supported(bn, B2, True, ch, max_c=None) is s2t_any
    assert bool(bev_train.bn_supported(bn, ch)) is bev
    assert bool(sp_train.bn_supported(bn, ch)) is sp
    assert bool(sa_train._bn_ok(bn)) is sa


def test_predicate_maximum_width():
    assert bn_train.supported(B2(128), B2, False, None, 128) and not bn_train.supported(B2(132), B2, False, None, 128)
    assert not bn_train.supported(B2(64, momentum=True), B2, False)          # a bool is no numeric momentum


def test_update_running_equals_batch_norms_own_update():
    """two modules share one fused call's batch_stats (ctot, off); one has no num_batches_tracked.  1e-6 relative: the fp32 rounding
    of the one multiply-add per element"""
    g = torch.Generator().manual_seed(5)
    rows, cs, moms = 96, (8, 12), (0.1, 0.01)
    ctot = sum(cs)
    xs = [2.0 + torch.randn(rows, c, generator=g) * (0.5 + torch.rand(c, generator=g)) for c in cs]
    x64 = torch.cat(xs, 1).double()
    batch_stats = torch.cat([x64.mean(0), x64.var(0, unbiased=False), x64.var(0, unbiased=True)]).float()
    nbts = [torch.tensor(3, dtype=torch.long), None]
    off = 0
    for x, c, m, nbt in zip(xs, cs, moms, nbts):
        rm0, rv0 = 0.5 + torch.rand(c, generator=g), 0.8 + 0.4 * torch.rand(c, generator=g)
        rm, rv, rm_ref, rv_ref = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
        versions = (rm._version, rv._version)
        bn_train.update_running(rm, rv, nbt, m, batch_stats, c, ctot=ctot, off=off)
        F.batch_norm(x, rm_ref, rv_ref, training=True, momentum=m)
        torch.testing.assert_close(rm, rm_ref, rtol=1e-6, atol=0)
        torch.testing.assert_close(rv, rv_ref, rtol=1e-6, atol=0)
        assert (rm._version, rv._version) == (versions[0] + 2, versions[1] + 2)       # mul_ and add_, as before
        off += c
    assert int(nbts[0]) == 4
    # one module on its own: ctot and off default to its width and 0
    rm, rv = torch.zeros(cs[0]), torch.ones(cs[0])
    rm_ref, rv_ref = rm.clone(), rv.clone()
    x64 = xs[0].double()
    own = torch.cat([x64.mean(0), x64.var(0, unbiased=False), x64.var(0, unbiased=True)]).float()
    bn_train.update_running(rm, rv, None, 0.1, own, cs[0])
    F.batch_norm(xs[0], rm_ref, rv_ref, training=True, momentum=0.1)
    torch.testing.assert_close(rm, rm_ref, rtol=1e-6, atol=0)
    torch.testing.assert_close(rv, rv_ref, rtol=1e-6, atol=0)
