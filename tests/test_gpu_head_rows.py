"""csrc/head_rows.hip (box / direction columns of the merged 1x1 head for a list of anchors) and the rows decode of
csrc/anchor_post.hip on the GPU, on the smallest shapes that can go wrong: bit equality between gathered and all-anchors mode, under
permutation, repetition, across frames and parts; the dot-product error bound against float64; decode bit-equal to lidar_decode_topk;
guard words around the outputs."""
import numpy as np
import pytest
import torch

from lidardetection_amd import anchor_post

pytestmark = pytest.mark.gpu

H, W = 5, 7
LOCS = H * W
GUARD = 64


def _case(C, A, bins, B=2, seed=0):
    """random map (B, H, W, C), merged head weight (C, N) [cls 3A | box 7A | dir bins*A] and bias, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    N = A * (3 + 7 + bins)
    x = torch.randn(B, H, W, C, generator=g)
    x[1, 2] = x[0, 1]                                       # the same rows in another frame (and, cut in two, another part)
    wt = torch.randn(C, N, generator=g) * 0.2
    b = torch.randn(N, generator=g)
    return x, wt, b, 3 * A, 3 * A + 7 * A


def _run(x, wt, b, A, bins, box_off, dir_off, idx, dev, parts=1):
    """head_rows on the map cut into `parts` buffers along the batch -> logits (B, k or all anchors, 7 + bins) on the device"""
    B = x.shape[0]
    xs = [p.contiguous().to(dev) for p in torch.chunk(x, parts, 0)]
    out = anchor_post.head_rows(xs, wt.to(dev), b.to(dev), A, box_off, dir_off, bins, None if idx is None else idx.to(dev), batch=B)
    return out


def _ref64(x, wt, b, A, bins, box_off, dir_off):
    """all-anchors logits in float64 with the terms of the error bound: -> ref (B, LOCS*A, 7+bins), sum |x_i w_i|, |bias|"""
    B, C = x.shape[0], x.shape[-1]
    cols = torch.tensor([[box_off + a * 7 + q for q in range(7)] + [dir_off + a * bins + q for q in range(bins)] for a in range(A)])
    xr = x.reshape(B, LOCS, C).double()
    w = wt.double()[:, cols.reshape(-1)]                                         # (C, A * nc)
    ref = (xr @ w + b.double()[cols.reshape(-1)]).reshape(B, LOCS * A, -1)
    mag = (xr.abs() @ w.abs()).reshape(B, LOCS * A, -1)
    return ref, mag, b.double()[cols.reshape(-1)].abs().reshape(1, A, -1).repeat(1, LOCS, 1)


@pytest.fixture(scope="module")
def all_anchor_runs(dev):
    """every case once in all-anchors mode (shared, never modified): name -> (inputs, logits on the CPU)"""
    out = {}
    for name, (C, A, bins) in {"c384": (384, 6, 2), "c20": (20, 6, 2), "c1024": (1024, 6, 2), "c1024_a1": (1024, 1, 0),
                               "a1_nobins": (384, 1, 0), "a8_bins4": (132, 8, 4)}.items():
        case = _case(C, A, bins, seed=len(out))
        out[name] = (case, A, bins, _run(*case[:3], A, bins, *case[3:], None, dev).cpu())
    return out


@pytest.mark.parametrize("name", ["c384", "c20", "c1024", "c1024_a1", "a1_nobins", "a8_bins4"])
def test_all_anchor_logits_within_the_dot_product_bound_of_fp64(all_anchor_runs, name):
    """|got - ref64| <= gamma * sum_i |x_i w_i| + |bias| * eps with gamma = (C + 8) 2^-24: the bound of a length-C fp32 dot product in
    any summation order (C - 1 additions + the rounding of each product, fused here, + the bias addition), nothing measured"""
    (x, wt, b, box_off, dir_off), A, bins, got = all_anchor_runs[name]
    C = x.shape[-1]
    ref, mag, babs = _ref64(x, wt, b, A, bins, box_off, dir_off)
    assert got.shape == ref.shape == (2, LOCS * A, 7 + bins)
    bound = (C + 8) * 2.0 ** -24 * mag + babs * 2.0 ** -24
    err = (got.double() - ref).abs()
    print(f"[head_rows {name}] max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the same rows in another frame: the same bits
    g = got.view(2, H, W, A, -1)
    assert torch.equal(g[1, 2].view(torch.int32), g[0, 1].view(torch.int32))


@pytest.mark.parametrize("name", ["c384", "c20", "c1024", "a1_nobins", "a8_bins4"])
def test_gathered_lists_are_bit_equal_to_all_anchor_mode(all_anchor_runs, dev, name):
    (x, wt, b, box_off, dir_off), A, bins, full = all_anchor_runs[name]
    n = LOCS * A
    g = torch.Generator().manual_seed(5)
    k = n + 13                                                                   # more slots than anchors: repeated indices
    idx = torch.randint(0, n, (2, k), generator=g)
    idx[:, 0], idx[:, 1], idx[:, -1], idx[:, 5] = 0, n - 1, n - 1, 0             # first and last anchor of each frame, twice
    got = _run(x, wt, b, A, bins, box_off, dir_off, idx, dev).cpu()
    want = torch.gather(full, 1, idx.unsqueeze(-1).expand(-1, -1, full.shape[-1]))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # any permutation of the list: the permuted output
    perm = torch.randperm(k, generator=g)
    got_p = _run(x, wt, b, A, bins, box_off, dir_off, idx[:, perm].contiguous(), dev).cpu()
    assert torch.equal(got_p.view(torch.int32), got[:, perm].view(torch.int32))
    # one part against the same data cut into two buffers, gathered and all anchors
    got_2 = _run(x, wt, b, A, bins, box_off, dir_off, idx, dev, parts=2).cpu()
    full_2 = _run(x, wt, b, A, bins, box_off, dir_off, None, dev, parts=2).cpu()
    assert torch.equal(got_2.view(torch.int32), got.view(torch.int32)) and torch.equal(full_2.view(torch.int32), full.view(torch.int32))


def test_guard_words_around_the_outputs_stay(dev):
    """the kernels write (B, k, 7 + bins) logits and (B, k, 7) boxes and nothing next to them: run them into the middle of larger
    buffers through the C ABI"""
    from lidardetection_amd import _lib
    from lidardetection_amd.pointpillar import generate_anchors
    from lidardetection_amd import synth
    A, bins, C = 6, 2, 384
    x, wt, b, box_off, dir_off = _case(C, A, bins, seed=9)
    k, nc = 11, 7 + bins
    idx = torch.randint(0, LOCS * A, (2, k), generator=torch.Generator().manual_seed(1)).to(dev)
    xd, wd, bd = x.to(dev), wt.to(dev), b.to(dev)
    buf = torch.full((GUARD + 2 * k * nc + GUARD,), -123.0, device=dev)
    L = _lib.lib()
    import ctypes
    _lib.check(L.lidar_head_rows(_lib.ptr(xd), None, 1, 2, LOCS, C, _lib.ptr(wd), wd.shape[1], _lib.ptr(bd), box_off, dir_off, A, bins,
                                 _lib.ptr(idx), 2, k, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), _lib.stream()), "lidar_head_rows")
    want = anchor_post.head_rows([xd], wd, bd, A, box_off, dir_off, bins, idx)
    assert torch.equal(buf[GUARD:-GUARD].view(2, k, nc), want)
    assert bool((buf[:GUARD] == -123.0).all()) and bool((buf[-GUARD:] == -123.0).all())
    anchors = generate_anchors(synth.PP_RANGE, (H, W), dev)
    bbuf = torch.full((GUARD + 2 * k * 7 + GUARD,), -123.0, device=dev)
    _lib.check(L.lidar_decode_topk_rows(_lib.ptr(want), 2, k, bins, _lib.ptr(idx), _lib.ptr(anchors), 0.78539, 0.0,
                                        float(np.float32(np.pi)), ctypes.c_void_p(bbuf.data_ptr() + 4 * GUARD), _lib.stream()),
               "lidar_decode_topk_rows")
    assert torch.equal(bbuf[GUARD:-GUARD].view(2, k, 7), anchor_post.decode_topk_rows(want, idx, anchors, bins, 0.78539, 0.0))
    assert bool((bbuf[:GUARD] == -123.0).all()) and bool((bbuf[-GUARD:] == -123.0).all())


@pytest.mark.parametrize("bins", [2, 0])
def test_rows_decode_is_bit_equal_to_decode_topk(dev, bins):
    """logits taken from a full head tensor -> lidar_decode_topk_rows == lidar_decode_topk on that tensor, as uint32"""
    from lidardetection_amd import synth
    from lidardetection_amd.pointpillar import generate_anchors
    A = 6
    g = torch.Generator().manual_seed(3 + bins)
    N = A * (3 + 7 + bins)
    head = torch.randn(2, H, W, N, generator=g)
    head[..., 3 * A:10 * A] *= 0.3
    head = head.to(dev)
    anchors = generate_anchors(synth.PP_RANGE, (H, W), dev)
    n = LOCS * A
    assert anchors.shape == (n, 7)
    idx = torch.randint(0, n, (2, n + 9), generator=g)
    idx[:, 0], idx[:, 1] = 0, n - 1
    idx = idx.to(dev)
    box_off, dir_off = 3 * A, 10 * A
    want = anchor_post.decode_topk(head, idx, anchors, A, box_off, dir_off, bins, 0.78539, 0.0)
    rows = head.view(2, LOCS, N)
    box = rows[..., box_off:box_off + 7 * A].reshape(2, n, 7)
    parts = [box] + ([rows[..., dir_off:dir_off + bins * A].reshape(2, n, bins)] if bins else [])
    logits = torch.gather(torch.cat(parts, -1), 1, idx.unsqueeze(-1).expand(-1, -1, 7 + bins)).contiguous()
    got = anchor_post.decode_topk_rows(logits, idx, anchors, bins, 0.78539, 0.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
