"""CPU checks of the sparse-conv entry points (csrc/sparse_conv.hip, csrc/rulebook_grid.hip): the support predicates against a
restatement of include/lidar_hip.h's sentences, every declared refusal from the outside (null or dummy host pointers and a null
stream: each check precedes the first HIP call of its entry point, so nothing is launched and nothing dereferenced), and the
CPU-side preconditions of the inputs tests/test_gpu_spconv_kernel_support.py feeds the kernels (tests/_spconv_np.py)."""
import ctypes as C

import numpy as np
import torch

import _spconv_np as sp
from lidardetection_amd import _lib

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
MFMA_C = (16, 32, 64, 128)


def _sorted_rule(K, cin, cout):
    return 1 <= K <= 32 and cin in MFMA_C and 1 <= cout <= 128 and cout % 4 == 0


def test_support_predicates_are_the_declared_rules():
    """lidar_spconv_sorted_gemm_supported, lidar_spconv_packed_floats, lidar_spconv_wgrad_mfma_supported over K in [-1, 40],
    Cin, Cout in [-1, 130]"""
    L = _lib.lib()
    srt, pk, wg = L.lidar_spconv_sorted_gemm_supported, L.lidar_spconv_packed_floats, L.lidar_spconv_wgrad_mfma_supported
    n_sorted = n_wgrad = 0
    for K in range(-1, 41):
        for cin in range(-1, 131):
            for cout in range(-1, 131):
                s = _sorted_rule(K, cin, cout)
                w = K > 0 and cin in MFMA_C and cout in MFMA_C
                assert srt(K, cin, cout) == int(s), (K, cin, cout)
                assert pk(K, cin, cout) == (K * cin * ((cout + 31) // 32) * 32 if s else 0), (K, cin, cout)
                assert wg(K, cin, cout) == int(w), (K, cin, cout)
                n_sorted += s
                n_wgrad += w
    assert n_sorted == 32 * 4 * 32 and n_wgrad == 40 * 16


def _dummy(nbytes=256):
    buf = C.create_string_buffer(nbytes + 32)
    addr = (C.addressof(buf) + 15) & ~15            # 16-byte aligned host address inside buf
    return buf, addr


def test_gemm_entry_points_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    buf, a = _dummy()
    p = C.c_void_p(a)
    fused = lambda n_out=10, K=27, cin=16, cout=16, ptr=p: L.lidar_spconv_implicit_gemm_fused(ptr, ptr, n_out, K, cin, cout, ptr, None, None, 0, ptr, None)   # noqa: E731
    plain = lambda n_out=10, K=27, cin=16, cout=16: L.lidar_spconv_implicit_gemm(p, p, n_out, K, cin, cout, p, None, p, None)   # noqa: E731
    for f in (fused, plain):
        for kw in (dict(cin=0), dict(cin=129), dict(cout=0), dict(cout=129), dict(K=0), dict(K=-1), dict(n_out=-1), dict(cin=-4)):
            assert f(**kw) == ERR_ARG, kw
            assert f(**dict(kw, n_out=kw.get("n_out", 0))) == ERR_ARG, kw               # refused even with nothing to do
    assert fused(n_out=0) == OK and plain(n_out=0) == OK and fused(n_out=0, cin=128, cout=127, K=125) == OK
    assert fused(ptr=None) == ERR_ARG                                                   # rows to compute: the null pointers are refused
    srt = lambda n_out=10, K=27, cin=16, cout=16, mask=p, order=p: L.lidar_spconv_implicit_gemm_sorted(                        # noqa: E731
        p, p, mask, order, n_out, K, cin, cout, p, None, None, 0, p, None)
    pkd = lambda n_out=10, K=27, cin=16, cout=16, mask=p, order=p, packed=p: L.lidar_spconv_implicit_gemm_sorted_packed(       # noqa: E731
        p, p, mask, order, n_out, K, cin, cout, packed, None, None, 0, p, None)
    for f in (srt, pkd):
        for kw in (dict(cin=5), dict(cin=4), dict(cout=18), dict(cout=132), dict(K=33), dict(K=0), dict(cin=0), dict(cout=0)):
            assert f(**kw) == ERR_ARG and f(**dict(kw, n_out=0)) == ERR_ARG, kw          # an unsupported shape
        assert f(mask=None) == ERR_ARG and f(order=None) == ERR_ARG and f(mask=None, order=None) == ERR_ARG
        assert f(n_out=-1) == ERR_ARG
        assert f(n_out=0) == OK and f(n_out=0, mask=None, order=None) == OK and f(n_out=0, K=32, cin=128, cout=128) == OK
    for off in (4, 8, 12):                                                              # a packed pointer that is not 16-byte aligned
        assert pkd(packed=C.c_void_p(a + off)) == ERR_ARG and pkd(n_out=0, packed=C.c_void_p(a + off)) == ERR_ARG
        assert L.lidar_spconv_pack_weights(p, 27, 16, 16, C.c_void_p(a + off), None) == ERR_ARG
    assert pkd(packed=None) == ERR_ARG
    assert L.lidar_spconv_pack_weights(p, 27, 5, 16, p, None) == ERR_ARG and L.lidar_spconv_pack_weights(p, 33, 16, 16, p, None) == ERR_ARG
    assert L.lidar_spconv_pack_weights(None, 27, 16, 16, p, None) == ERR_ARG
    del buf


def test_mask_entry_points_refuse_the_outside_of_their_declared_range():
    """the K limits of the mask-ordered route as the header lists them: row_masks K <= 32, mask_group K <= 31"""
    L = _lib.lib()
    buf, a = _dummy()
    p = C.c_void_p(a)
    assert L.lidar_spconv_row_masks(p, 10, 33, p, None) == ERR_ARG and L.lidar_spconv_row_masks(p, 0, 33, p, None) == ERR_ARG
    assert L.lidar_spconv_row_masks(p, 10, 0, p, None) == ERR_ARG and L.lidar_spconv_row_masks(p, -1, 27, p, None) == ERR_ARG
    assert L.lidar_spconv_row_masks(None, 10, 32, p, None) == ERR_ARG and L.lidar_spconv_row_masks(p, 0, 32, p, None) == OK
    mg = lambda n_out=10, K=27, ws=p, wsb=1 << 30: L.lidar_spconv_mask_group(p, n_out, K, p, p, ws, wsb, None)               # noqa: E731
    assert mg(K=32) == ERR_ARG and mg(K=32, n_out=0) == ERR_ARG and mg(K=0) == ERR_ARG and mg(n_out=-1) == ERR_ARG
    assert mg(ws=None) == ERR_ARG and mg(n_out=0, K=31) == OK
    assert mg(wsb=1024) == ERR_WORKSPACE                                                # smaller than the smallest table
    assert L.lidar_spconv_mask_group_init(p, 1024, None) == ERR_WORKSPACE and L.lidar_spconv_mask_group_init(None, 1 << 30, None) == ERR_WORKSPACE
    assert L.lidar_spconv_mask_group_workspace_bytes(1) == L.lidar_spconv_mask_group_workspace_bytes(1 << 15)
    assert L.lidar_spconv_mask_group_workspace_bytes((1 << 15) + 1) > L.lidar_spconv_mask_group_workspace_bytes(1 << 15)
    del buf


def test_wgrad_entry_points_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    buf, a = _dummy()
    p = C.c_void_p(a)
    wg = lambda n_out=10, K=27, cin=16, cout=16, ptr=p: L.lidar_spconv_wgrad(ptr, ptr, ptr, n_out, K, cin, cout, ptr, None)   # noqa: E731
    for kw in (dict(cin=0), dict(cin=129), dict(cout=0), dict(cout=129), dict(K=0), dict(n_out=-1)):
        assert wg(**kw) == ERR_ARG and wg(**dict(kw, n_out=kw.get("n_out", 0))) == ERR_ARG, kw
    assert wg(n_out=0) == OK and wg(n_out=0, cin=127, cout=128, K=125) == OK and wg(ptr=None) == ERR_ARG
    wm = lambda n_out=300, K=27, cin=16, cout=16, gw=p, ws=p, wsb=0: L.lidar_spconv_wgrad_mfma(p, p, p, None, n_out, K, cin, cout, gw, ws, wsb, None)   # noqa: E731
    for kw in (dict(cin=5), dict(cin=48), dict(cout=36), dict(cout=4), dict(K=0), dict(n_out=-1), dict(gw=None), dict(ws=None)):
        assert wm(**kw) == ERR_ARG, kw
    for n_out, K, cin, cout in ((300, 27, 16, 16), (1, 1, 128, 128), (5000, 32, 64, 32)):
        need = L.lidar_spconv_wgrad_workspace_bytes(n_out, K, cin, cout)
        chunks = min(128, max(1, -(-n_out // 1024)))
        assert need == K * chunks * cin * cout * 4
        assert wm(n_out=n_out, K=K, cin=cin, cout=cout, wsb=need - 1) == ERR_WORKSPACE   # a workspace one byte short
        assert wm(n_out=n_out, K=K, cin=cin, cout=cout, wsb=0) == ERR_WORKSPACE
    del buf


def test_rulebook_entry_points_refuse_the_outside_of_their_declared_range():
    """a hash capacity that is not a power of two (or below 2 n), kernel / stride / extent <= 0, and a padded input thinner than
    the kernel (the C division truncates: 2 planes, kernel 3, stride 2 would otherwise report one output plane)"""
    L = _lib.lib()
    buf, a = _dummy()
    p = C.c_void_p(a)
    assert L.lidar_spconv_hash_capacity(0) == 1024 and L.lidar_spconv_hash_capacity(512) == 1024 and L.lidar_spconv_hash_capacity(513) == 2048
    for cap in (1000, 1023, 1025, 3 << 10):
        assert L.lidar_spconv_build_hash(p, 0, 4, 4, 4, p, cap, None) == ERR_ARG, cap
    assert L.lidar_spconv_build_hash(p, 600, 4, 4, 4, p, 1024, None) == ERR_ARG          # a power of two below 2 n
    assert L.lidar_spconv_build_hash(p, -1, 4, 4, 4, p, 1024, None) == ERR_ARG and L.lidar_spconv_build_hash(p, 0, 4, 4, 4, None, 1024, None) == ERR_ARG

    def outputs(shape, k, s, pd, n=10, batch=2, num=p):
        return L.lidar_spconv_conv_outputs(p, n, batch, *shape, *k, *s, *pd, p, 1 << 20, num, p, 1 << 30, None)

    def grid_outputs(shape, k, s, pd, n=10, batch=2, num=p):
        return L.lidar_spconv_grid_outputs(p, n, batch, *shape, *k, *s, *pd, p, p, num, p, 1 << 30, None)

    def grid_table(shape, k, s, pd, n=10, batch=2):
        return L.lidar_spconv_grid_table(p, n, batch, *shape, *k, *s, *pd, p, 0, p, None)

    thin = [([2, 8, 8], [3, 3, 3], [2, 2, 2], [0, 0, 0]), ([1, 8, 8], [3, 3, 3], [1, 1, 1], [0, 0, 0]), ([8, 8, 1], [2, 2, 2], [2, 2, 2], [0, 0, 0]),
            ([8, 2, 8], [3, 5, 3], [1, 4, 1], [1, 1, 1]), ([8, 8, 8], [3, 3, 3], [0, 1, 1], [1, 1, 1]), ([8, 8, 8], [3, 0, 3], [1, 1, 1], [1, 1, 1]),
            ([0, 8, 8], [1, 1, 1], [1, 1, 1], [0, 0, 0]), ([0, 8, 8], [2, 1, 1], [1, 1, 1], [1, 0, 0]), ([8, 8, -1], [1, 1, 1], [1, 1, 1], [0, 0, 1])]
    for shape, k, s, pd in thin:
        for f in (outputs, grid_outputs, grid_table):
            assert f(shape, k, s, pd) == ERR_ARG and f(shape, k, s, pd, n=0) == ERR_ARG, (f.__name__, shape, k, s, pd)
    for f in (outputs, grid_outputs):
        assert f([8, 8, 8], [3, 3, 3], [2, 2, 2], [1, 1, 1], n=-1) == ERR_ARG and f([8, 8, 8], [3, 3, 3], [2, 2, 2], [1, 1, 1], batch=0) == ERR_ARG
        assert f([8, 8, 8], [3, 3, 3], [2, 2, 2], [1, 1, 1], num=None) == ERR_ARG
    assert grid_table([1, 12, 12], [3, 3, 3], [1, 1, 1], [1, 1, 1], n=0) == OK           # an extent of 1 WITH padding is a geometry like any other
    assert grid_table([2, 3, 2], [3, 3, 3], [2, 2, 2], [1, 1, 1], n=0) == OK and grid_table([8, 8, 8], [2, 2, 2], [2, 2, 2], [0, 0, 0], n=0) == OK
    assert L.lidar_spconv_subm_table(p, 10, 4, 4, 4, 3, 0, 3, p, 1024, p, None) == ERR_ARG
    assert L.lidar_spconv_subm_table(p, -1, 4, 4, 4, 3, 3, 3, p, 1024, p, None) == ERR_ARG
    assert L.lidar_spconv_subm_table(p, 0, 4, 4, 4, 3, 3, 3, p, 1024, p, None) == OK
    del buf


def test_gpu_test_inputs_meet_their_preconditions():
    """every committed case of tests/_spconv_np.py: the exact regime's sums stay below 2**22 in magnitude with values that are
    multiples of 0.5 (so any summation order is exact in fp32), the blank patterns are blank and nothing else is, every column that
    is not blanked on purpose is used, unreferenced input rows (and only those) are NaN, and the tables index inside the inputs"""
    specs = sp.specs()
    assert len(specs) > 200
    for cin, cout, n_out, K, kw in specs:
        d = sp.exact_inputs(sp.SEED, cin, cout, n_out, K, **kw)
        nbr = d["nbr"].numpy()
        assert nbr.shape == (n_out, K) and nbr.dtype == np.int32 and nbr.min() >= -1 and nbr.max() < sp.N_IN
        blank = sp.blank_rows(n_out)
        live = np.setdiff1d(np.arange(n_out), blank)
        assert (nbr[blank] == -1).all()
        if n_out >= 256:
            assert set(range(32, 64)) <= set(blank) and set(range(128, 256)) <= set(blank) and 7 in blank
        col_used = (nbr >= 0).any(0)
        for k in range(K):
            assert col_used[k] == (k != kw.get("blank_col")), (cin, cout, n_out, K, k)
        if K == 32 and kw.get("blank_col") is None:
            assert int(sp.masks_of(d["nbr"]).max()) >= 1 << 31                          # bit 31 set: the mask is negative as an int32
        if live.size > 40 and K >= 8:
            assert ((nbr[live] >= 0).sum(1) > 0).mean() > 0.9                           # the live rows are live
        used = np.zeros(sp.N_IN, bool)
        used[nbr[nbr >= 0]] = True
        feats = d["feats"].numpy()
        assert not used[-sp.N_SPARE:].any() and (~used).sum() >= sp.N_SPARE              # the NaN trap is set at every shape
        assert np.isnan(feats[~used]).all() and np.isfinite(feats[used]).all()
        for name in ("feats", "w", "bias", "res", "go"):
            v = d[name].numpy()
            v = v[np.isfinite(v)]
            assert (v * 2 == np.round(v * 2)).all() and np.abs(v).max(initial=0) <= 8, name
        assert np.abs(d["feats"].numpy()[used]).max(initial=0) <= 3 and np.abs(d["w"].numpy()).max() <= 2
        assert float(sp.abs_bound(d["feats"], d["nbr"], d["w"], d["bias"], d["res"]).max()) < 2 ** 22
        assert float(sp.wgrad_abs_bound(d["feats"], d["go"], d["nbr"], K).max()) < 2 ** 22
        ref = sp.gemm_ref(d["feats"], d["nbr"], d["w"], d["bias"], d["res"], True)
        assert bool(torch.isfinite(ref).all()) and torch.equal(ref.float().double(), ref)   # the reference itself is an fp32 number
        if kw.get("injective"):
            for k in range(K):
                col = nbr[:, k][nbr[:, k] >= 0]
                assert len(np.unique(col)) == len(col)
            t = sp.transposed(d["nbr"], sp.N_IN).numpy()
            i, k = np.nonzero(t >= 0)
            assert (nbr[t[i, k], k] == i).all() and (t >= 0).sum() == (nbr >= 0).sum()


def test_reference_formulas_on_a_hand_computed_case():
    """gemm_ref / wgrad_ref / abs_bound / gauss_tol on numbers small enough to do by hand"""
    feats = torch.tensor([[1.0, 2.0], [3.0, -1.0], [float("nan"), float("nan")]])
    nbr = torch.tensor([[0, 1], [-1, 0], [-1, -1]], dtype=torch.int32)
    w = torch.tensor([[[1.0], [0.5]], [[-2.0], [1.0]]])                                  # (K 2, Cin 2, Cout 1)
    bias, res = torch.tensor([1.0]), torch.tensor([[0.0], [-5.0], [2.0]])
    out = sp.gemm_ref(feats, nbr, w, bias, res, False)
    assert out.tolist() == [[1 + 1 - 6 - 1 + 1], [-2 + 2 + 1 - 5], [1 + 2]]
    assert sp.gemm_ref(feats, nbr, w, bias, res, True).tolist() == [[0.0], [0.0], [3.0]]
    assert sp.abs_bound(feats, nbr, w, bias, res).tolist() == [[1 + 1 + 6 + 1 + 1], [2 + 2 + 1 + 5], [1 + 2]]
    assert sp.n_terms(nbr, 2).tolist() == [[4], [2], [0]]
    go = torch.tensor([[2.0], [1.0], [7.0]])
    assert sp.wgrad_ref(feats, go, nbr, 2).tolist() == [[[2.0], [4.0]], [[6 + 1.0], [-2 + 2.0]]]
    assert sp.wgrad_abs_bound(feats, go, nbr, 2).tolist() == [[[2.0], [4.0]], [[7.0], [4.0]]]
    assert sp.wgrad_n_terms(nbr).reshape(-1).tolist() == [1, 2]
    assert sp.gauss_tol(np.array([[4]]), np.array([[10.0]])).tolist() == [[6 * 2.0 ** -23 * 10.0]]
    assert sp.masks_of(nbr).tolist() == [3, 2, 0]
