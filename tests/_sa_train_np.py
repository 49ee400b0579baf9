"""float64 numpy replay of the train-mode set-abstraction kernels (csrc/sa_train.hip (a)-(d)) and of one whole scale, plus the
fixtures the host and GPU tests share.  `idx` (the raw ball-query result) and `arg` (the chosen sample of the max) are INPUTS: the
replay states what the kernels must compute given them; the choice itself is checked separately."""
import numpy as np


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample):
    """the raw stacked ball query: the first nsample sources of the query's frame within the radius, in index order (indices
    within the frame), padded with the first hit; an empty ball is -1 in column 0 and 0 elsewhere"""
    idx = np.zeros((len(new_xyz), nsample), np.int32)
    xs, qs = np.concatenate(([0], np.cumsum(xyz_cnt))), np.concatenate(([0], np.cumsum(new_cnt)))
    for b in range(len(xyz_cnt)):
        pts = xyz[xs[b]:xs[b + 1]].astype(np.float32)
        for m in range(qs[b], qs[b + 1]):
            d = pts - new_xyz[m].astype(np.float32)
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            hit = np.nonzero(d2 < np.float32(radius) * np.float32(radius))[0][:nsample]
            if len(hit) == 0:
                idx[m, 0] = -1
            else:
                idx[m, :] = hit[0]
                idx[m, :len(hit)] = hit
    return idx


def cloud(seed, xyz_cnt, new_cnt, width):
    """sources in a 4 m cube per frame, queries partly on sources (full / padded balls) and partly far outside (empty balls)"""
    r = np.random.default_rng(seed)
    N, M = int(sum(xyz_cnt)), int(sum(new_cnt))
    xyz = r.uniform(0, 4, (N, 3)).astype(np.float32)
    feats = r.standard_normal((N, width)).astype(np.float32)
    new_xyz = r.uniform(0, 4, (M, 3)).astype(np.float32)
    far = r.random(M) < 0.25
    far[:1] = False                                          # never query 0: at M = 1 the batch would be all zero rows (variance 0)
    new_xyz[far] += 50.0                                     # empty balls
    return xyz, feats, new_xyz


CASES = [   # (seed, xyz_cnt, new_cnt, nsample, H, radius)
    (1, [60], [1], 8, 4, 1.0),
    (2, [40, 0, 300], [1, 1, 1], 1, 16, 0.8),
    (3, [120, 90, 0], [70, 0, 60], 16, 64, 0.9),
    (4, [300], [130], 64, 128, 1.6),
    (5, [100, 250, 77], [40, 50, 40], 8, 128, 0.5),
    (6, [150], [3], 16, 16, 1.2),
]


# ---- (a) - (c) -----------------------------------------------------------------------------------------------------------------------
def _starts(xyz_cnt, new_cnt):
    xs = np.concatenate(([0], np.cumsum(xyz_cnt)))[:-1]
    return np.repeat(xs, new_cnt).astype(np.int64)             # start of each query's frame in the sources


def pair_keys(idx, xyz_cnt, new_cnt, N):
    """global source row of every pair; N for the pairs of empty balls"""
    M, ns = idx.shape
    key = _starts(xyz_cnt, new_cnt)[:, None] + idx.astype(np.int64)
    key[idx[:, 0] < 0] = N
    return key.reshape(-1)


def gather_forward(table, query_term, idx, xyz_cnt, new_cnt):
    M, ns = idx.shape
    N, H = table.shape
    key = pair_keys(idx, xyz_cnt, new_cnt, N)
    z = np.zeros((M * ns, H), np.float64)
    live = key < N
    z[live] = table.astype(np.float64)[key[live]]
    if query_term is not None:
        z[live] -= np.repeat(query_term.astype(np.float64), ns, axis=0)[live]
    return z


def inverse_index(idx, xyz_cnt, new_cnt, N):
    key = pair_keys(idx, xyz_cnt, new_cnt, N)
    pairs = np.argsort(key, kind="stable").astype(np.int32)
    row_start = np.searchsorted(key[pairs], np.arange(N + 1), side="left").astype(np.int32)
    return row_start, pairs


def gather_backward(dz, idx, xyz_cnt, new_cnt, N):
    M, ns = idx.shape
    key = pair_keys(idx, xyz_cnt, new_cnt, N)
    dz = dz.astype(np.float64)
    d_table = np.zeros((N + 1, dz.shape[1]), np.float64)
    np.add.at(d_table, key, dz)
    d_query = -dz.reshape(M, ns, -1).sum(1)
    d_query[idx[:, 0] < 0] = 0
    return d_table[:N], d_query


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------
def bn_stats(z, eps):
    mu, var = z.mean(0), z.var(0)
    return mu, var, 1.0 / np.sqrt(var + eps)


def bn_relu_max_forward(z, M, ns, gamma, beta, eps, arg):
    """-> (out (M, H) read at `arg`, y (M, ns, H), pre-activation (M, ns, H), (mu, biased var, unbiased var))"""
    z = z.astype(np.float64)
    mu, var, inv = bn_stats(z, eps)
    pre = ((z - mu) * inv * gamma.astype(np.float64) + beta.astype(np.float64)).reshape(M, ns, -1)
    y = np.maximum(pre, 0)
    out = np.take_along_axis(y, arg.astype(np.int64)[:, None, :], axis=1)[:, 0]
    n = z.shape[0]
    return out, y, pre, (mu, var, var * n / (n - 1))


def bn_relu_max_backward(z, M, ns, grad_out, arg, gamma, beta, eps):
    z = z.astype(np.float64)
    mu, var, inv = bn_stats(z, eps)
    zh = (z - mu) * inv
    pre = (zh * gamma + beta).reshape(M, ns, -1)
    delta = np.zeros_like(pre)
    a = arg.astype(np.int64)[:, None, :]
    g = grad_out.astype(np.float64)[:, None, :] * (np.take_along_axis(pre, a, axis=1) > 0)
    np.put_along_axis(delta, a, g, axis=1)
    delta = delta.reshape(z.shape)
    d_beta, d_gamma = delta.sum(0), (delta * zh).sum(0)
    n = z.shape[0]
    dz = gamma * inv * (delta - d_beta / n - zh * d_gamma / n)
    return dz, d_gamma, d_beta


def bn_relu_rows(z, gamma, beta, eps):
    mu, var, inv = bn_stats(z, eps)
    zh = (z - mu) * inv
    return np.maximum(zh * gamma + beta, 0), zh, inv


def bn_relu_rows_backward(gy, y, zh, inv, gamma):
    delta = gy * (y > 0)
    d_beta, d_gamma = delta.sum(0), (delta * zh).sum(0)
    n = zh.shape[0]
    return gamma * inv * (delta - d_beta / n - zh * d_gamma / n), d_gamma, d_beta


# ---- one whole scale -----------------------------------------------------------------------------------------------------------------
def scale_replay(xyz, feats, new_xyz, idx, xyz_cnt, new_cnt, weights, gammas, betas, eps, grad_out, arg):
    """A scale [xyz | feats] -> weights[0] -> BN/ReLU -> ... -> weights[-1] -> BN/ReLU -> max, forward and backward, in float64.
    weights[k] (H_k, C_k); arg (M, H_last) the chosen samples -> dict(out, d_feats, d_w, d_gamma, d_beta, pre_last)"""
    f64 = lambda a: np.asarray(a, np.float64)                 # noqa: E731
    xyz, feats, new_xyz = f64(xyz), f64(feats), f64(new_xyz)
    W = [f64(w) for w in weights]
    G, Bt = [f64(g) for g in gammas], [f64(b) for b in betas]
    M, ns = idx.shape
    N = xyz.shape[0]
    src = np.concatenate((xyz, feats), 1)
    table, query = src @ W[0].T, new_xyz @ W[0][:, :3].T
    z = gather_forward(table, query, idx, xyz_cnt, new_cnt)
    saved, zs = [], [z]
    for k in range(1, len(W)):
        y, zh, inv = bn_relu_rows(zs[-1], G[k - 1], Bt[k - 1], eps)
        saved.append((y, zh, inv))
        zs.append(y @ W[k].T)
    out, _, pre, _ = bn_relu_max_forward(zs[-1], M, ns, G[-1], Bt[-1], eps, arg)
    d_w, d_g, d_b = [None] * len(W), [None] * len(W), [None] * len(W)
    dz, d_g[-1], d_b[-1] = bn_relu_max_backward(zs[-1], M, ns, f64(grad_out), arg, G[-1], Bt[-1], eps)
    for k in range(len(W) - 1, 0, -1):
        y, zh, inv = saved[k - 1]
        d_w[k] = dz.T @ y
        dz, d_g[k - 1], d_b[k - 1] = bn_relu_rows_backward(dz @ W[k], y, zh, inv, G[k - 1])
    d_table, d_query = gather_backward(dz, idx, xyz_cnt, new_cnt, N)
    d_w[0] = d_table.T @ src
    d_w[0][:, :3] += d_query.T @ new_xyz
    return dict(out=out, d_feats=(d_table @ W[0])[:, 3:], d_w=d_w, d_gamma=d_g, d_beta=d_b, pre_last=pre)


def reference_arg(pre):
    """the lowest sample index among the maxima of relu(pre) (M, ns, H) in float64: max_pool2d's choice"""
    return np.argmax(np.maximum(pre, 0), axis=1).astype(np.uint8)
