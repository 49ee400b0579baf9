"""Plain float64 restatement of the sparse-conv GEMM and weight gradient (csrc/sparse_conv.hip) and the seeded CPU inputs of
tests/test_gpu_spconv_kernel_support.py.  No GPU, no library call: tests/test_spconv_kernel_args_host.py asserts the
preconditions stated here (exactness bound, blank patterns, every column used) for every seed the GPU tests use.

    out[j]  = act(sum_k feats[nbr[j, k]] @ w[k] + bias + residual[j])          over the k with nbr[j, k] >= 0
    dW[k]   = sum_j feats[nbr[j, k]]^T (x) grad_out[j]                         over the j with nbr[j, k] >= 0

Two data regimes:
  exact  features are integers in [-3, 3], weights come from {-2, -1, -0.5, 0, 0.5, 1, 2}, bias / residual / grad_out are
         integers in [-8, 8].  Every product is a multiple of 0.5 and every partial sum, in ANY order, is a multiple of 0.5
         below 2**22 in magnitude (asserted: abs_bound < 2**22; 32 * 128 * 6 = 24 576 for K <= 32, C <= 128), hence exactly
         representable in fp32 (24 significant bits).  A kernel that drops, doubles or misplaces one product differs by at
         least 0.5 whatever its summation order: the GPU result must be torch.equal to the reference.
  gauss  features ~ N(0, 1), weights ~ 0.2 N(0, 1): sees a precision change (a reduced-precision matrix-core path) that the
         integers cannot.  Per-element tolerance GAUSS_TOL (below).

Input rows no table entry refers to are NaN in `feats` (the last N_SPARE rows are never drawn, so there are some at every
shape): a kernel that multiplies a missing neighbour by zero instead of skipping or zero-filling it shows up as NaN in its output.
"""
import functools

import numpy as np
import torch

N_IN = 300
N_SPARE = 8                        # the last input rows are never drawn by the table generator: NaN at every shape
EXACT_W = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
EXACT_LIMIT = float(2 ** 22)
# Forward error of an fp32 sum of n products, each product and each addition rounded once with unit roundoff u = 2**-24:
# |fl(s) - s| <= gamma_n * sum|a||w| with gamma_n = n u / (1 - n u) ~ n u (Higham, Accuracy and Stability of Numerical Algorithms,
# section 3.1); the epilogue adds bias and residual: two more roundings, hence n_terms + 2.  The matrix core's v_mfma_f32_32x32x2
# step adds TWO products to the accumulator and is not documented as rounding that step once, so u is doubled: 2**-23.
GAUSS_U = 2.0 ** -23


def gauss_tol(n_terms, bound):
    """(n_terms + 2) * 2**-23 * abs_bound, elementwise (n_terms broadcasts over the channel axes)"""
    return (np.asarray(n_terms, np.float64) + 2.0) * GAUSS_U * np.asarray(bound, np.float64)


def blank_rows(n_out, row=True, wave=True, workgroup=True):
    """rows the table generator empties: one row (row 7, inside a tile whose other rows are live; n_out // 2 for tiny tables), rows
    [32, 64) — a whole 32-row wave tile — and rows [128, 256) — a whole 128-row workgroup; each only where it fits below n_out"""
    rows = []
    if row and n_out >= 3:
        rows.append(7 if n_out > 8 else n_out // 2)
    if wave:
        rows += list(range(32, min(64, n_out)))
    if workgroup:
        rows += list(range(128, min(256, n_out)))
    return sorted(set(rows))


@functools.lru_cache(maxsize=None)
def _table(seed, n_out, K, n_in, p, row, wave, workgroup, blank_col, injective):
    r = np.random.default_rng(seed)
    if injective:      # every column is a partial injection rows -> input rows: the table has a transposed table
        assert n_out <= n_in - N_SPARE
        nbr = np.stack([r.permutation(n_in - N_SPARE)[:n_out] for _ in range(K)], 1).astype(np.int32)
    else:
        nbr = r.integers(0, n_in - N_SPARE, (n_out, K)).astype(np.int32)
    nbr[r.random((n_out, K)) >= p] = -1
    blank = blank_rows(n_out, row, wave, workgroup)
    live = np.setdiff1d(np.arange(n_out), blank)
    nbr[blank] = -1
    if blank_col is not None:
        nbr[:, blank_col] = -1
    # every column that is not blanked on purpose is used by at least one live row (K = 32: bit 31 is really set somewhere);
    # a column without any entry stays injective with one
    for k in range(K):
        if k != blank_col and live.size and not (nbr[:, k] >= 0).any():
            nbr[live[(k * 7) % live.size], k] = (k * 13 + 5) % (n_in - N_SPARE)
    nbr.setflags(write=False)
    return nbr


def table(seed, n_out, K, n_in=N_IN, p=0.4, row=True, wave=True, workgroup=True, blank_col=None, injective=False):
    """(n_out, K) int32 neighbour table over n_in input rows, each entry valid with probability p; blank_rows(...) emptied;
    blank_col: an offset used by no row at all.  Cached and read-only."""
    if blank_col is not None and blank_col >= K:
        blank_col = None
    return _table(seed, n_out, K, n_in, p, bool(row), bool(wave), bool(workgroup), blank_col, bool(injective))


def _nan_unreferenced(feats, nbr):
    used = np.zeros(feats.shape[0], bool)
    used[nbr[nbr >= 0]] = True
    feats[~used] = np.nan
    return feats


@functools.lru_cache(maxsize=None)
def _inputs(regime, seed, cin, cout, nbr_key):
    nbr = _table(*nbr_key)
    n_out, K = nbr.shape
    n_in = nbr_key[3]
    r = np.random.default_rng(seed * 7919 + cin * 131 + cout)
    if regime == "exact":
        feats = r.integers(-3, 4, (n_in, cin)).astype(np.float32)
        w = r.choice(np.asarray(EXACT_W, np.float32), (K, cin, cout))
        bias = r.integers(-8, 9, (cout,)).astype(np.float32)
        res = r.integers(-8, 9, (n_out, cout)).astype(np.float32)
        go = r.integers(-8, 9, (n_out, cout)).astype(np.float32)
    else:
        feats = r.standard_normal((n_in, cin)).astype(np.float32)
        w = (0.2 * r.standard_normal((K, cin, cout))).astype(np.float32)
        bias = r.standard_normal((cout,)).astype(np.float32)
        res = r.standard_normal((n_out, cout)).astype(np.float32)
        go = r.standard_normal((n_out, cout)).astype(np.float32)
    feats = _nan_unreferenced(feats, nbr)
    d = {"nbr": torch.from_numpy(nbr.copy()), "feats": torch.from_numpy(feats), "w": torch.from_numpy(w), "bias": torch.from_numpy(bias),
         "res": torch.from_numpy(res), "go": torch.from_numpy(go)}
    if regime == "exact":
        assert float(abs_bound(d["feats"], d["nbr"], d["w"], d["bias"], d["res"]).max()) < EXACT_LIMIT
        assert float(wgrad_abs_bound(d["feats"], d["go"], d["nbr"], K).max(initial=0.0)) < EXACT_LIMIT
    return d


def _key(seed, n_out, K, n_in=N_IN, p=0.4, row=True, wave=True, workgroup=True, blank_col=None, injective=False):
    if blank_col is not None and blank_col >= K:
        blank_col = None
    return (seed, n_out, K, n_in, p, bool(row), bool(wave), bool(workgroup), blank_col, bool(injective))


def exact_inputs(seed, cin, cout, n_out, K, **table_kw):
    """seeded exact-regime inputs (see the module docstring): dict of CPU tensors nbr, feats, w, bias, res, go.  Shared between
    tests (cached): treat as read-only."""
    return _inputs("exact", seed, cin, cout, _key(seed, n_out, K, **table_kw))


def gauss_inputs(seed, cin, cout, n_out, K, **table_kw):
    """seeded Gaussian-regime inputs: the same dict"""
    return _inputs("gauss", seed, cin, cout, _key(seed, n_out, K, **table_kw))


def _gather(feats, nbr, k):
    """float64 (n_out, Cin): the gathered rows of offset k, exact zeros where the neighbour is missing (never NaN * 0)"""
    col = nbr[:, k].long()
    a = torch.zeros((nbr.shape[0], feats.shape[1]), dtype=torch.float64)
    m = col >= 0
    a[m] = feats[col[m]].double()
    return a


def gemm_ref(feats, nbr, w, bias=None, residual=None, relu=False):
    """float64 (n_out, Cout)"""
    out = torch.zeros((nbr.shape[0], w.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[1]):
        out += _gather(feats, nbr, k) @ w[k].double()
    if bias is not None:
        out = out + bias.double()
    if residual is not None:
        out = out + residual.double()
    return torch.relu(out) if relu else out


def abs_bound(feats, nbr, w, bias=None, residual=None):
    """sum |a| |w| + |bias| + |residual| per output element, float64 (n_out, Cout)"""
    out = torch.zeros((nbr.shape[0], w.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[1]):
        out += _gather(feats, nbr, k).abs() @ w[k].double().abs()
    if bias is not None:
        out = out + bias.double().abs()
    if residual is not None:
        out = out + residual.double().abs()
    return out.numpy()


def n_terms(nbr, cin):
    """valid (offset, channel) products per output row, (n_out, 1)"""
    return ((nbr >= 0).sum(1, keepdim=True) * cin).numpy()


def wgrad_ref(feats, grad_out, nbr, K):
    """float64 (K, Cin, Cout)"""
    return torch.stack([_gather(feats, nbr, k).t() @ (grad_out.double() * (nbr[:, k:k + 1] >= 0)) for k in range(K)])


def wgrad_abs_bound(feats, grad_out, nbr, K):
    return torch.stack([_gather(feats, nbr, k).abs().t() @ (grad_out.double().abs() * (nbr[:, k:k + 1] >= 0)) for k in range(K)]).numpy()


def wgrad_n_terms(nbr):
    """valid rows per offset, (K, 1, 1)"""
    return (nbr >= 0).sum(0).numpy().reshape(-1, 1, 1)


def transposed(nbr, n_in):
    """nbr_t (n_in, K): nbr[j, k] == i  <=>  nbr_t[i, k] == j (the table must be injective per column)"""
    t = torch.full((n_in, nbr.shape[1]), -1, dtype=torch.int32)
    j, k = torch.nonzero(nbr >= 0, as_tuple=True)
    t[nbr[j, k].long(), k] = j.int()
    return t


def masks_of(nbr):
    """int64 (n_out): bit k = nbr[., k] >= 0"""
    return ((nbr >= 0).long() << torch.arange(nbr.shape[1])).sum(1)


# ---------------------------------------------------------------------------------------------- the committed cases
# One seed; tests/test_gpu_spconv_kernel_support.py runs these, tests/test_spconv_kernel_args_host.py asserts the preconditions
# of the module docstring on every one of them (specs()).
SEED = 20
BLANK_COL = 5                      # the offset nobody uses (tables with K > 5)
N_STD = 257                        # two workgroups + one row: blank row 7, blank wave [32, 64), blank workgroup [128, 256)
EPILOGUES = ((True, True, 1), (False, False, 0), (True, False, 1))          # (bias, residual, relu)
REGA_SHAPES = [(ci, co) for ci in (16, 32, 64, 128) for co in (4, 20, 32, 36, 64, 68, 96, 100, 128)]
GENERIC_SHAPES = [(1, 1), (3, 7), (5, 33), (7, 65), (8, 16), (12, 97), (20, 126), (100, 30), (127, 128), (128, 126), (128, 127),
                  (16, 5), (64, 1), (4, 65), (4, 128)]
INPUT_SHAPES = [(4, co, K) for co in (1, 4, 31, 32, 33, 63, 64) for K in (1, 27, 28)] + [(4, 16, 29)]
K_SWEEP_SHAPES = [(32, 36), (5, 33)]
K_SWEEP = (1, 2, 3, 8, 9, 28, 29, 31, 32)
ROW_EDGE_SHAPES = [(32, 36), (128, 20), (5, 33), (4, 33)]
ROW_EDGES = (1, 31, 32, 33, 127, 128, 129, 255, 256)
SORTED_SHAPES = [(ci, co) for ci in (16, 32, 64, 128) for co in (4, 36, 68, 100, 128)]
SORTED_K = (3, 27, 31, 32)         # 32: through lidar_spconv_row_masks + argsort, every column used (no blank column)
SWITCH_SHAPES = [(16, 20), (32, 36), (64, 68), (64, 128), (128, 36), (128, 128)]
SWITCH_ALL_SHAPES = SWITCH_SHAPES + [s for s in SORTED_SHAPES if s not in SWITCH_SHAPES]    # + every (NT, Cin) instance of the two kernels
WGRAD_SCALAR_SHAPES = [(5, 16), (20, 48), (33, 100), (100, 80), (127, 128), (128, 128), (1, 1)]     # PER 1, 4, 16, 32, 64, 64, 1
WGRAD_MFMA_SHAPES = [(ci, co) for ci in (16, 32, 64, 128) for co in (16, 32, 64, 128)]
WGRAD_K = (1, 27, 32)
WGRAD_ROWS = (1, 127, 128, 129, 511, 512, 513)
WGRAD_ROW_SHAPES = {"scalar": (33, 100), "mfma": (64, 32)}
WGRAD_TWO_CHUNKS = 1025            # the MFMA kernel splits the rows into chunks of >= 1024: the smallest count with two partials to sum
BACKWARD_SHAPES = [(5, 33), (32, 36)]
# LIDAR_SPCONV_RT2=1: sc_implicit_gemm_rega2_kernel<NT, C4> is selected for Cin 32 / 64, Cout <= 64 and n_out >= 2048 (16 row tiles of 128)
RT2_SHAPES = [(32, 16), (64, 32), (32, 36), (64, 64)]           # <1, 8>, <1, 16>, <2, 8>, <2, 16>
RT2_ROWS = 2049
RT2_K = (27, 32)


def std_table_kw(K):
    return {"blank_col": BLANK_COL if K > BLANK_COL else None}


def specs():
    """every (cin, cout, n_out, K, table keywords) the GPU tests build inputs for"""
    out = []
    for ci, co in REGA_SHAPES + GENERIC_SHAPES + SWITCH_SHAPES:
        out.append((ci, co, N_STD, 27, std_table_kw(27)))
    for ci, co, K in INPUT_SHAPES:
        out.append((ci, co, N_STD, K, std_table_kw(K)))
    for ci, co in K_SWEEP_SHAPES:
        out += [(ci, co, N_STD, K, std_table_kw(K)) for K in K_SWEEP]
    for ci, co in ROW_EDGE_SHAPES:
        out += [(ci, co, n, 27, std_table_kw(27)) for n in ROW_EDGES]
    for ci, co in SORTED_SHAPES:
        out += [(ci, co, N_STD, K, std_table_kw(K) if K < 32 else {}) for K in SORTED_K]
    for ci, co in WGRAD_SCALAR_SHAPES + WGRAD_MFMA_SHAPES:
        out += [(ci, co, N_STD, K, std_table_kw(K)) for K in WGRAD_K]
    for ci, co in WGRAD_ROW_SHAPES.values():
        out += [(ci, co, n, 27, std_table_kw(27)) for n in WGRAD_ROWS + (WGRAD_TWO_CHUNKS,)]
    for ci, co in RT2_SHAPES:
        out += [(ci, co, RT2_ROWS, K, std_table_kw(K) if K < 32 else {}) for K in RT2_K]
    for ci, co in BACKWARD_SHAPES:
        out.append((ci, co, N_STD, 27, dict(std_table_kw(27), injective=True)))
    seen, uniq = set(), []
    for s in out:
        key = (s[0], s[1], s[2], s[3], tuple(sorted(s[4].items())))
        if key not in seen:
            seen.add(key)
            uniq.append(s)
    return uniq


def child_cases(which):
    """(cin, cout, n_out, K, table keywords) a child process of the GPU tests runs: "switch" (pipe / wave kernels) or "rt2" """
    if which == "switch":
        return [(ci, co, N_STD, 27, std_table_kw(27)) for ci, co in SWITCH_ALL_SHAPES]
    return [(ci, co, RT2_ROWS, K, std_table_kw(K) if K < 32 else {}) for ci, co in RT2_SHAPES for K in RT2_K]
