"""The sparse-conv GEMM, weight-gradient and rulebook kernels (csrc/sparse_conv.hip, csrc/rulebook_grid.hip, spconv/ops.py) over
the support include/lidar_hip.h declares — Cin, Cout <= 128, any K > 0 — against the float64 restatement tests/_spconv_np.py.

Every kernel template sc_gemm_launch, lidar_spconv_wgrad and lidar_spconv_wgrad_mfma can select is run: the register-A kernel
(NT 1..4 x Cin 16 / 32 / 64 / 128-in-two-slices), the generic kernel (NT 1..4, scalar and float4 staging, odd Cin, the 131 584-byte
LDS corner), the input-layer kernel, the packed-weight kernel, the switch-selected pipe and wave kernels (child processes), the
scalar wgrad (PER 1 / 4 / 16 / 32 / 64) and all 16 MFMA wgrad shapes; row counts around the 32-row wave tile, the 128-row workgroup
and the 512-row wgrad chunk; tables with an empty row, an empty wave, an empty workgroup and an offset nobody uses.

Two data regimes (tests/_spconv_np.py): `exact` — small integers and halves, every partial sum exactly representable, the result
must be torch.equal to the reference whatever the summation order; `gauss` — within (n_terms + 2) * 2**-23 * sum|a||w|.
Output buffers carry one extra row and arrive filled with a sentinel: the extra row must survive, no sentinel may remain.
Rulebooks: both builders against the brute-force oracle (oracle/spconv_oracle.py) on even kernels, mixed strides, stride 3, grids
thinner than the kernel, sites on every face and corner, a single site, a full grid, batch 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _spconv_np as sp
from lidardetection_amd import _lib, spconv, workspace
from lidardetection_amd.spconv import ops
from oracle import spconv_oracle as so

pytestmark = pytest.mark.gpu

SENT = 777.0
REGIMES = ("exact", "gauss")
FULL_TERMS = 16      # an element with at least this many summed products is a real accumulation chain, not one or two roundings
RATIOS = {}          # kernel family -> [largest Gaussian-regime error / tolerance over all elements, over those with >= FULL_TERMS terms]


@pytest.fixture(scope="module", autouse=True)
def _report_gauss_ratios():
    """one summary line per kernel family when the module is done (visible with pytest -s)"""
    yield
    for family, (every, full) in sorted(RATIOS.items()):
        print(f"\nGAUSS_RATIO {family}: all elements {every:.4f}, elements with >= {FULL_TERMS} terms {full:.4f}")


def _inputs(regime, cin, cout, n_out, K, **kw):
    return (sp.exact_inputs if regime == "exact" else sp.gauss_inputs)(sp.SEED, cin, cout, n_out, K, **kw)


def _on(dev, d):
    return {k: v.to(dev) for k, v in d.items()}


def _gemm(dev, g, epi, order=None, packed=None):
    """one raw call into an (n_out + 1, Cout) sentinel buffer -> rows [0, n_out)"""
    L = _lib.lib()
    n_out, K = g["nbr"].shape
    _, cin, cout = g["w"].shape
    bias = g["bias"] if epi[0] else None
    res = g["res"] if epi[1] else None
    buf = torch.full((n_out + 1, cout), SENT, device=dev)
    if packed is not None:
        st = L.lidar_spconv_implicit_gemm_sorted_packed(_lib.ptr(g["feats"]), _lib.ptr(g["nbr"]), _lib.ptr(order[0]), _lib.ptr(order[1]),
                                                        n_out, K, cin, cout, _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res), epi[2],
                                                        _lib.ptr(buf), _lib.stream())
    elif order is not None:
        st = L.lidar_spconv_implicit_gemm_sorted(_lib.ptr(g["feats"]), _lib.ptr(g["nbr"]), _lib.ptr(order[0]), _lib.ptr(order[1]), n_out,
                                                 K, cin, cout, _lib.ptr(g["w"]), _lib.ptr(bias), _lib.ptr(res), epi[2], _lib.ptr(buf),
                                                 _lib.stream())
    else:
        st = L.lidar_spconv_implicit_gemm_fused(_lib.ptr(g["feats"]), _lib.ptr(g["nbr"]), n_out, K, cin, cout, _lib.ptr(g["w"]),
                                                _lib.ptr(bias), _lib.ptr(res), epi[2], _lib.ptr(buf), _lib.stream())
    _lib.check(st, f"sparse GEMM {cin} -> {cout}, K {K}, n_out {n_out}")
    assert bool((buf[n_out] == SENT).all()), "the row past the output was written"
    return buf[:n_out]


def _ref(d, epi):
    return sp.gemm_ref(d["feats"], d["nbr"], d["w"], d["bias"] if epi[0] else None, d["res"] if epi[1] else None, bool(epi[2]))


def _check(got, ref, regime, family, n_terms=None, bound=None):
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), "NaN / inf in the output: a missing neighbour was read"
    assert not bool(((got == SENT) & (ref != SENT)).any()), "an output element was never written"
    if regime == "exact":
        bad = got != ref.float()
        assert not bool(bad.any()), (family, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
        return
    err = (got.double() - ref).abs().numpy()
    tol = sp.gauss_tol(n_terms, bound)
    rel = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
    full = np.broadcast_to(np.asarray(n_terms) >= FULL_TERMS, rel.shape)
    seen = RATIOS.setdefault(family, [0.0, 0.0])
    seen[0] = max(seen[0], float(rel.max(initial=0.0)))
    seen[1] = max(seen[1], float(rel[full].max(initial=0.0)))
    assert bool((err <= tol).all()), (family, float(rel.max(initial=0.0)))


def _gemm_case(dev, family, cin, cout, n_out, K, epilogues=sp.EPILOGUES, regimes=REGIMES, **kw):
    for regime in regimes:
        d = _inputs(regime, cin, cout, n_out, K, **kw)
        g = _on(dev, d)
        for epi in epilogues:
            got = _gemm(dev, g, epi)
            bound = sp.abs_bound(d["feats"], d["nbr"], d["w"], d["bias"] if epi[0] else None, d["res"] if epi[1] else None)
            _check(got, _ref(d, epi), regime, family, sp.n_terms(d["nbr"], cin), bound)


# ------------------------------------------------------------------------------------------------ a. GEMM route table
@pytest.mark.parametrize("cin,cout", sp.REGA_SHAPES)
def test_register_a_kernel_route(dev, cin, cout):
    """sc_implicit_gemm_rega_kernel<NT 1..4, C4 4 / 8 / 16, SL 1 / 2>: one, two, three and four column tiles, Cout a multiple of 4
    but not of 16, Cin 128 in two slices with a narrow Cout"""
    assert _lib.lib().lidar_spconv_sorted_gemm_supported(27, cin, cout) == 1            # (the register-A predicate)
    _gemm_case(dev, "rega", cin, cout, sp.N_STD, 27, **sp.std_table_kw(27))


@pytest.mark.parametrize("cin,cout", sp.GENERIC_SHAPES)
def test_generic_kernel_route(dev, cin, cout):
    """sc_implicit_gemm_kernel<NT 1..4>: scalar W staging (Cout % 4 != 0), scalar gather and the odd-Cin guard, float4 gather
    outside {16, 32, 64, 128}; (128, 126), (128, 127) and (127, 128) launch with 131 584 / 130 560 bytes of dynamic LDS"""
    assert _lib.lib().lidar_spconv_sorted_gemm_supported(27, cin, cout) == 0
    _gemm_case(dev, "generic", cin, cout, sp.N_STD, 27, **sp.std_table_kw(27))


@pytest.mark.parametrize("cin,cout,K", sp.INPUT_SHAPES)
def test_input_layer_kernel_route(dev, cin, cout, K):
    """sc_input_layer_gemm_kernel<1 / 2> (Cin 4, K <= 28, Cout <= 64); K = 29 falls to the generic kernel"""
    _gemm_case(dev, "input" if K <= 28 else "generic", cin, cout, sp.N_STD, K, **sp.std_table_kw(K))


@pytest.mark.parametrize("K", sp.K_SWEEP)
@pytest.mark.parametrize("cin,cout", sp.K_SWEEP_SHAPES)
def test_gemm_offset_counts(dev, cin, cout, K):
    """K 1 .. 32 on one register-A and one generic shape (K = 32: offset 31 is the sign bit of a row mask)"""
    _gemm_case(dev, "rega" if cin == 32 else "generic", cin, cout, sp.N_STD, K, **sp.std_table_kw(K))


# ------------------------------------------------------------------------------------------------ b. row edges
@pytest.mark.parametrize("n_out", sp.ROW_EDGES)
@pytest.mark.parametrize("cin,cout", sp.ROW_EDGE_SHAPES)
def test_gemm_row_count_edges(dev, cin, cout, n_out):
    """row counts around the 32-row wave tile and the 128-row workgroup, exact regime"""
    fam = {32: "rega", 128: "rega", 5: "generic", 4: "input"}[cin]
    _gemm_case(dev, fam, cin, cout, n_out, 27, regimes=("exact",), **sp.std_table_kw(27))


@pytest.mark.parametrize("cin,cout", sp.ROW_EDGE_SHAPES)
def test_gemm_of_no_rows_launches_nothing(dev, cin, cout):
    L = _lib.lib()
    g = _on(dev, _inputs("exact", cin, cout, 1, 27, **sp.std_table_kw(27)))
    buf = torch.full((1, cout), SENT, device=dev)
    assert L.lidar_spconv_implicit_gemm_fused(_lib.ptr(g["feats"]), _lib.ptr(g["nbr"]), 0, 27, cin, cout, _lib.ptr(g["w"]), _lib.ptr(g["bias"]),
                                              _lib.ptr(g["res"]), 1, _lib.ptr(buf), _lib.stream()) == 0
    assert bool((buf == SENT).all())


# ------------------------------------------------------------------------------------------------ c. mask-ordered and packed routes
def _orders(dev, nbr_d, K):
    """-> {name: (masks, order)}: the mask order (lidar_spconv_mask_group for K <= 31, lidar_spconv_row_masks + argsort at 32), the
    identity and the reversed order"""
    n_out = nbr_d.shape[0]
    if K <= 31:
        masks, order = ops.mask_order(nbr_d)
    else:
        masks = torch.empty(n_out, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().lidar_spconv_row_masks(_lib.ptr(nbr_d), n_out, K, _lib.ptr(masks), _lib.stream()), "lidar_spconv_row_masks")
        order = torch.argsort(masks).int()
    want = sp.masks_of(nbr_d.cpu())
    assert torch.equal(masks.cpu().long() & 0xFFFFFFFF, want)
    assert torch.equal(torch.sort(order.cpu().long()).values, torch.arange(n_out))
    ident = torch.arange(n_out, dtype=torch.int32, device=dev)
    return {"mask": (masks, order), "identity": (masks, ident), "reversed": (masks, ident.flip(0).contiguous())}


@pytest.mark.parametrize("K", sp.SORTED_K)
@pytest.mark.parametrize("cin,cout", sp.SORTED_SHAPES)
def test_mask_ordered_and_packed_routes(dev, cin, cout, K):
    """lidar_spconv_implicit_gemm_sorted (register-A kernel with row masks) and ..._sorted_packed (sc_implicit_gemm_pk_kernel): the
    bits of the table-order call in both regimes, exact against float64; identity and reversed orders give the same bits"""
    L = _lib.lib()
    assert L.lidar_spconv_sorted_gemm_supported(K, cin, cout) == 1
    assert ops.sorted_gemm_supported(K, cin, cout) == (K <= 31)
    kw = sp.std_table_kw(K) if K < 32 else {}
    keep = ops.PACKED_GEMM[0]
    for regime in REGIMES:
        d = _inputs(regime, cin, cout, sp.N_STD, K, **kw)
        if K == 32:
            assert bool((d["nbr"] >= 0).any(0).all())                              # every column used: bit 31 is set in some mask
        g = _on(dev, d)
        orders = _orders(dev, g["nbr"], K)
        ops.PACKED_GEMM[0] = True
        try:
            packed = ops.pack_gemm_weights(g["w"])
        finally:
            ops.PACKED_GEMM[0] = keep
        assert packed is not None and packed.numel() == L.lidar_spconv_packed_floats(K, cin, cout) == K * cin * ((cout + 31) // 32) * 32
        for epi in sp.EPILOGUES:
            base = _gemm(dev, g, epi)
            bound = sp.abs_bound(d["feats"], d["nbr"], d["w"], d["bias"] if epi[0] else None, d["res"] if epi[1] else None)
            _check(base, _ref(d, epi), regime, "rega", sp.n_terms(d["nbr"], cin), bound)
            for name, order in orders.items():
                assert torch.equal(_gemm(dev, g, epi, order), base), ("sorted", name, regime, epi)
                assert torch.equal(_gemm(dev, g, epi, order, packed), base), ("packed", name, regime, epi)


# ------------------------------------------------------------------------------------------------ d. switch-selected kernels
_CHILD = r"""
import sys, torch
import _spconv_np as sp
from lidardetection_amd.spconv import ops
from lidardetection_amd import _lib
dev = torch.device("cuda:0")
outs = {}
for cin, cout, n_out, K, kw in sp.child_cases(sys.argv[2]):
    d = sp.exact_inputs(sp.SEED, cin, cout, n_out, K, **kw)
    g = {k: v.to(dev) for k, v in d.items()}
    if K <= 31:
        st = ops.mask_order(g["nbr"])
    else:                                    # K = 32: lidar_spconv_row_masks + a sort of the signed masks
        masks = torch.empty(n_out, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().lidar_spconv_row_masks(_lib.ptr(g["nbr"]), n_out, K, _lib.ptr(masks), _lib.stream()), "lidar_spconv_row_masks")
        st = (masks, torch.argsort(masks).int())
    for name, order in (("table", None), ("mask", st)):
        outs[f"{cin}-{cout}-{K}-{name}-full"] = ops.indice_conv_fused(g["feats"], g["nbr"], g["w"], g["bias"], g["res"], True, order).cpu()
        outs[f"{cin}-{cout}-{K}-{name}-plain"] = ops.indice_conv_fused(g["feats"], g["nbr"], g["w"], None, None, False, order).cpu()
torch.cuda.synchronize()
torch.save(outs, sys.argv[1])
"""


def _child(tmp_path, switch, which):
    """one fresh interpreter with `switch` set runs sp.child_cases(which) in table and mask order -> its outputs, checked against
    float64.  A child that dies is a finding, not something to run again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "child.pt")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.environ.get("PYTHONPATH", "")]))
    for name in ("LIDAR_SPCONV_PIPE_KERNEL", "LIDAR_SPCONV_WAVE_KERNEL", "LIDAR_SPCONV_RT2"):
        env.pop(name, None)
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, out, which], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, (switch, r.returncode, r.stderr[-2000:])
    outs = torch.load(out, weights_only=True)
    cases = sp.child_cases(which)
    assert len(outs) == 4 * len(cases)
    for cin, cout, n_out, K, kw in cases:
        d = sp.exact_inputs(sp.SEED, cin, cout, n_out, K, **kw)
        full, plain = _ref(d, (True, True, 1)).float(), _ref(d, (False, False, 0)).float()
        for name in ("table", "mask"):
            assert torch.equal(outs[f"{cin}-{cout}-{K}-{name}-full"], full), (switch, cin, cout, K, name)
            assert torch.equal(outs[f"{cin}-{cout}-{K}-{name}-plain"], plain), (switch, cin, cout, K, name)


@pytest.mark.parametrize("switch", ["LIDAR_SPCONV_PIPE_KERNEL", "LIDAR_SPCONV_WAVE_KERNEL"])
def test_switch_selected_gemm_kernels(dev, tmp_path, switch):
    """sc_implicit_gemm_pipe_kernel / sc_implicit_gemm_wave_kernel: compiled in, chosen by an environment variable read once per
    process -> one fresh child interpreter per switch runs the exact regime in table and mask order, the parent compares with
    float64.  The shapes reach every <NT 1..4, Cin 16 / 32 / 64 / 128-in-two-slices> instance of the pipe kernel and every <NT 1..2,
    Cin 16 / 32 / 64> instance of the wave kernel (which needs 4 x Cin x 32 NT floats <= 64 KB of LDS); the other shapes exercise
    the wave switch's fall-back to the default kernel."""
    _child(tmp_path, switch, "switch")


def test_two_row_tile_kernel_instances(dev, tmp_path):
    """LIDAR_SPCONV_RT2=1: sc_implicit_gemm_rega2_kernel<1, 8>, <1, 16>, <2, 8>, <2, 16> ((32, 16), (64, 32), (32, 36), (64, 64)) —
    selected only from 2048 rows on, hence 2049 rows here (16 row tiles of 128 and one row) — exact against float64 in table and
    mask order, at K = 27 and at K = 32, where the kernel reads offset 31 out of the sign bit of the row masks"""
    _child(tmp_path, "LIDAR_SPCONV_RT2", "rt2")


# ------------------------------------------------------------------------------------------------ e. weight gradients
def _wgrad_scalar(dev, g, cin, cout):
    n_out, K = g["nbr"].shape
    gw = torch.zeros((K + 1, cin, cout), device=dev)
    gw[K] = SENT
    _lib.check(_lib.lib().lidar_spconv_wgrad(_lib.ptr(g["feats"]), _lib.ptr(g["go"]), _lib.ptr(g["nbr"]), n_out, K, cin, cout, _lib.ptr(gw),
                                             _lib.stream()), "lidar_spconv_wgrad")
    assert bool((gw[K] == SENT).all())
    return gw[:K]


def _wgrad_mfma(dev, g, cin, cout, order):
    L = _lib.lib()
    n_out, K = g["nbr"].shape
    wsb = L.lidar_spconv_wgrad_workspace_bytes(n_out, K, cin, cout)
    ws = workspace.get("spconv_wgrad_support_test", wsb, dev)
    gw = torch.full((K + 1, cin, cout), float("nan"), device=dev)
    gw[K] = SENT
    _lib.check(L.lidar_spconv_wgrad_mfma(_lib.ptr(g["feats"]), _lib.ptr(g["go"]), _lib.ptr(g["nbr"]), _lib.ptr(order), n_out, K, cin, cout,
                                         _lib.ptr(gw), _lib.ptr(ws), wsb, _lib.stream()), "lidar_spconv_wgrad_mfma")
    assert bool((gw[K] == SENT).all())
    return gw[:K]


def _wgrad_case(dev, kind, cin, cout, n_out, K):
    kw = sp.std_table_kw(K)
    for regime in REGIMES:
        d = _inputs(regime, cin, cout, n_out, K, **kw)
        g = _on(dev, d)
        ref = sp.wgrad_ref(d["feats"], d["go"], d["nbr"], K)
        nt, bound = sp.wgrad_n_terms(d["nbr"]), sp.wgrad_abs_bound(d["feats"], d["go"], d["nbr"], K)
        if kind == "scalar":
            runs = [_wgrad_scalar(dev, g, cin, cout)]
        else:
            assert _lib.lib().lidar_spconv_wgrad_mfma_supported(K, cin, cout) == 1
            order = ops.mask_order(g["nbr"])[1] if K <= 31 else None             # K = 32: order = NULL
            runs = [_wgrad_mfma(dev, g, cin, cout, o) for o in (None, order, None)]
            assert torch.equal(runs[0], runs[2]), "two runs of the MFMA weight gradient differ"
        for got in runs:
            _check(got, ref, regime, "wgrad_" + kind, nt, bound)
            if kw["blank_col"] is not None:
                assert bool((got[kw["blank_col"]] == 0).all()), "the gradient of an offset nobody uses is not zero"


@pytest.mark.parametrize("K", sp.WGRAD_K)
@pytest.mark.parametrize("cin,cout", sp.WGRAD_SCALAR_SHAPES)
def test_scalar_wgrad_templates(dev, cin, cout, K):
    """sc_wgrad_kernel<PER 1 / 4 / 16 / 32 / 64> (float atomics): exact in the exact regime whatever the order of the atomics"""
    _wgrad_case(dev, "scalar", cin, cout, sp.N_STD, K)


@pytest.mark.parametrize("K", sp.WGRAD_K)
@pytest.mark.parametrize("cin,cout", sp.WGRAD_MFMA_SHAPES)
def test_mfma_wgrad_shapes(dev, cin, cout, K):
    """sc_wgrad_mfma_kernel<NTI, NTO> for all 16 (Cin, Cout) pairs, with and without the mask order; grad_weight arrives as NaN"""
    _wgrad_case(dev, "mfma", cin, cout, sp.N_STD, K)


@pytest.mark.parametrize("n_out", sp.WGRAD_ROWS + (sp.WGRAD_TWO_CHUNKS,))
@pytest.mark.parametrize("kind", ["scalar", "mfma"])
def test_wgrad_row_count_edges(dev, kind, n_out):
    """row counts around the 128-row MFMA tile and the 512-row chunk of the scalar kernel; 1025 rows are the MFMA kernel's first
    count with two chunk partials for its reduce kernel to sum (three workgroups along the rows for the scalar kernel)"""
    cin, cout = sp.WGRAD_ROW_SHAPES[kind]
    _wgrad_case(dev, kind, cin, cout, n_out, 27)


@pytest.mark.parametrize("cin,cout", sp.BACKWARD_SHAPES)
def test_conv_function_backward_is_exact(dev, cin, cout):
    """SparseConvFunction.backward end to end in the exact regime: y = relu(conv(f, w, b) + residual), grad_feats (implicit GEMM over
    the transposed table, 33 -> 5 and 36 -> 32), grad_w (the scalar kernel: neither shape has an MFMA weight gradient) and grad_b
    against float64 autograd of the reference formula — exact"""
    K = 27
    d = sp.exact_inputs(sp.SEED, cin, cout, sp.N_STD, K, injective=True, **sp.std_table_kw(K))
    nbr, feats = d["nbr"], torch.nan_to_num(d["feats"], nan=0.0)     # (a leaf with NaN rows would have NaN * 0 in torch's own relu chain)
    nbr_t = sp.transposed(nbr, sp.N_IN)
    f = feats.to(dev).requires_grad_(True)
    w = d["w"].to(dev).requires_grad_(True)
    b = d["bias"].to(dev).requires_grad_(True)
    y = torch.relu(ops.indice_conv(f, w.view(3, 3, 3, cin, cout), b, nbr.to(dev), nbr_t.to(dev), False) + d["res"].to(dev))
    y.backward(d["go"].to(dev))
    fd, wd, bd = (t.double().requires_grad_(True) for t in (feats, d["w"], d["bias"]))
    out = torch.zeros((sp.N_STD, cout), dtype=torch.float64)
    for k in range(K):
        m = nbr[:, k] >= 0
        out = out.index_add(0, torch.nonzero(m)[:, 0], fd[nbr[m, k].long()] @ wd[k])
    yr = torch.relu(out + bd + d["res"].double())
    yr.backward(d["go"].double())
    assert torch.equal(y.detach().cpu(), yr.detach().float())
    assert torch.equal(f.grad.cpu(), fd.grad.float())
    assert torch.equal(w.grad.cpu(), wd.grad.float())
    assert torch.equal(b.grad.cpu(), bd.grad.float())


# ------------------------------------------------------------------------------------------------ f. rulebooks
REGULAR_GEOMS = [([8, 8, 8], [2, 2, 2], [2, 2, 2], [0, 0, 0]), ([9, 10, 11], [3, 3, 3], [1, 2, 2], [1, 1, 1]),
                 ([9, 9, 9], [3, 3, 3], [3, 3, 3], [0, 0, 0]), ([1, 12, 12], [3, 3, 3], [1, 1, 1], [1, 1, 1]),
                 ([2, 3, 2], [3, 3, 3], [2, 2, 2], [1, 1, 1]), ([6, 7, 8], [1, 3, 3], [1, 2, 2], [0, 1, 1]),
                 ([6, 6, 6], [3, 3, 3], [1, 1, 1], [0, 0, 0]), ([7, 7, 7], [3, 3, 3], [2, 2, 2], [2, 2, 2])]
SUBM_KERNELS = [[3, 3, 3], [1, 3, 3], [3, 1, 1], [5, 5, 5]]
SUBM_SHAPE = [6, 7, 8]


def _occupancies(shape, B):
    """name -> (n, 4) int32 [b, z, y, x]: corners + face centres, a single site, the full grid, 35 % random, the same with one
    duplicated coordinate"""
    D, H, W = shape
    zs, ys, xs = (0, D - 1), (0, H - 1), (0, W - 1)
    pts = [(z, y, x) for z in zs for y in ys for x in xs]
    pts += [(z, H // 2, W // 2) for z in zs] + [(D // 2, y, W // 2) for y in ys] + [(D // 2, H // 2, x) for x in xs]
    pts = sorted(set(pts))
    occ = {"corners+faces": np.array([(b, *p) for b in range(B) for p in pts], np.int32),
           "single": np.array([(B - 1, D - 1, H // 2, 0)], np.int32)}
    cells = np.array([(b, z, y, x) for b in range(B) for z in range(D) for y in range(H) for x in range(W)], np.int32)
    r = np.random.default_rng(B * 1000 + D * 100 + H * 10 + W)
    if B == 1:
        occ["full"] = cells[r.permutation(len(cells))]
    rnd = cells[r.permutation(len(cells))[:max(2, int(0.35 * len(cells)))]]
    occ["random"] = rnd
    dup = rnd.copy()
    dup[len(dup) - 1] = dup[0]                                      # one duplicated coordinate: the lowest row wins
    occ["duplicate"] = dup
    return occ


def _triples(nbr, in_idx, out_idx):
    j, k = np.nonzero(nbr >= 0)
    return {(int(kk), tuple(int(v) for v in in_idx[nbr[jj, kk]]), tuple(int(v) for v in out_idx[jj])) for jj, kk in zip(j, k)}


def _build(coords, B, shape, ks, st, pd, subm, grid):
    keep = ops.GridPool.ENABLED
    ops.GridPool.ENABLED = grid
    try:
        if subm:
            return (ops.subm_rulebook(coords, shape, ks, B, {}),)
        return ops.conv_rulebook(coords, B, shape, ks, st, pd, {})
    finally:
        ops.GridPool.ENABLED = keep


def _rulebook_case(dev, shape, ks, st, pd, subm):
    for B in (1, 3):
        for name, idx in _occupancies(shape, B).items():
            coords = torch.from_numpy(idx).to(dev)
            res = {grid: _build(coords, B, shape, ks, st, pd, subm, grid) for grid in (True, False)}
            for a, b in zip(res[True], res[False]):
                assert torch.equal(a, b), (shape, ks, st, pd, B, name, "grid and hash builders differ")
            trip_o, outs_o = so.rulebook(idx, shape, ks, st, pd, subm)
            if subm:
                nbr = res[True][0].cpu().numpy()
                out_idx = idx
            else:
                out_idx, nbr, nbr_t = (t.cpu().numpy() for t in res[True])
                assert sorted(tuple(int(v) for v in r) for r in out_idx) == outs_o, (shape, ks, B, name)
                i, k = np.nonzero(nbr_t >= 0)
                tt = {(int(kk), tuple(int(v) for v in idx[ii]), tuple(int(v) for v in out_idx[nbr_t[ii, kk]])) for ii, kk in zip(i, k)}
                assert tt == trip_o, (shape, ks, B, name, "nbr_t")
                if name == "duplicate":    # in nbr_t every row of a coordinate, the losing one included, names the outputs it reaches
                    assert (nbr_t[len(idx) - 1] == nbr_t[0]).all() and (idx[len(idx) - 1] == idx[0]).all()
            assert nbr.shape == (len(out_idx), ks[0] * ks[1] * ks[2])
            assert _triples(nbr, idx, out_idx) == trip_o, (shape, ks, B, name, "nbr")
            if name == "duplicate":
                assert not bool((nbr == len(idx) - 1).any()), "the higher row of a duplicated coordinate is in the table"


@pytest.mark.parametrize("geom", REGULAR_GEOMS, ids=lambda g: "-".join("".join(str(v) for v in p) for p in g))
def test_regular_rulebooks_against_brute_force(dev, geom):
    """even kernels, mixed strides, stride 3, grids thinner than the kernel, an output level of the input level's shape: both
    builders, equal tensors, triples / output set / transposed table equal to the brute-force enumeration"""
    _rulebook_case(dev, *geom, False)


@pytest.mark.parametrize("ks", SUBM_KERNELS, ids=lambda k: "".join(str(v) for v in k))
def test_subm_rulebooks_against_brute_force(dev, ks):
    _rulebook_case(dev, SUBM_SHAPE, ks, [1, 1, 1], [k // 2 for k in ks], True)


@pytest.mark.parametrize("subm", [False, True])
def test_module_features_against_dense_convolution(dev, subm):
    """5 -> 33 through the module on exact-regime data: the float64 dense convolution after casting, within 1e-9"""
    shape, ks, st, pd = ([9, 10, 11], [3, 3, 3], [1, 2, 2], [1, 1, 1]) if not subm else (SUBM_SHAPE, [3, 3, 3], [1, 1, 1], [1, 1, 1])
    B, cin, cout = 3, 5, 33
    idx = _occupancies(shape, B)["random"]
    r = np.random.default_rng(3)
    feats = r.integers(-3, 4, (len(idx), cin)).astype(np.float32)
    mod = (spconv.SubMConv3d if subm else spconv.SparseConv3d)(cin, cout, ks, stride=st, padding=pd, bias=True).to(dev)
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(r.choice(np.asarray(sp.EXACT_W, np.float32), tuple(mod.weight.shape))))
        mod.bias.copy_(torch.from_numpy(r.integers(-8, 9, (cout,)).astype(np.float32)))
    y = mod(spconv.SparseConvTensor(torch.from_numpy(feats).to(dev), torch.from_numpy(idx).to(dev), shape, B))
    ref = so.conv_features(feats, idx, B, shape, mod.weight.detach().cpu(), mod.bias.detach().cpu(), ks, st, pd, subm, y.indices.cpu().numpy())
    assert float((y.features.detach().cpu().double() - ref).abs().max()) <= 1e-9


@pytest.mark.parametrize("shape,ks,st,pd", [([2, 8, 8], [3, 3, 3], [2, 2, 2], [0, 0, 0]), ([1, 8, 8], [3, 3, 3], [1, 1, 1], [0, 0, 0]),
                                            ([8, 8, 1], [2, 2, 2], [2, 2, 2], [0, 0, 0])])
def test_a_grid_thinner_than_the_unpadded_kernel_is_refused(dev, shape, ks, st, pd):
    """include/lidar_hip.h: a regular convolution whose padded input is thinner than its kernel along an axis has no output site;
    both builders refuse it with LIDAR_ERR_ARG (status -1) instead of numbering sites of a level that does not exist"""
    coords = torch.from_numpy(_occupancies(shape, 2)["random"]).to(dev)
    assert min(so.out_shape(shape, ks, st, pd)) <= 0
    for grid in (True, False):
        with pytest.raises(_lib.LidarHipError, match="status -1"):
            _build(coords, 2, shape, ks, st, pd, False, grid)
