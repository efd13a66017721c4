"""Plain numpy statements of gs2m_icp_step and gs2m_voxel_mean (include/gs2mesh_amd.h, gs2mesh_amd/csrc/icp_kernels.h).

icp_step: p = T s in f64 operation by operation, the f32 search rule of gs2m_nn_dist2 (nn_statement) on f32(p - o) against
f32(target - o), the f64 keep rule, and the sums in the kernel's stated order: thread t of workgroup b adds the indices
1024 b + t + 256 k (k = 0..3) from +0, a wave's 64 lanes by the halving tree, the four waves left to right, the workgroups'
partials t, t + 256, ... by thread t of a last workgroup that is reduced the same way.  numpy adds element by element in f64
and never contracts, so every line below is the arithmetic it looks like."""
import numpy as np

import nn_statement

THREADS, PER_THREAD = 256, 4
CHUNK = THREADS * PER_THREAD
N_SUMS = 17                                                   # the f64 sums; the pair count is an integer beside them


def transform(T, s):
    T = np.asarray(T, np.float64).reshape(4, 4)
    s = np.asarray(s, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3] for k in range(3)], 1)


def wave_tree(v):
    """[64, K] -> [K]: a = v[0:32] + v[32:64], a = a[0:16] + a[16:32], ..."""
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:h] + v[h:2 * h]
    return v[0]


def block_reduce(v):
    """[256, K] -> [K]"""
    w = [wave_tree(v[64 * u:64 * u + 64]) for u in range(THREADS // 64)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def reduce_terms(terms):
    """[N, K] f64, zero rows where the pair is not kept -> [K] in the kernel's order"""
    N, K = terms.shape
    blocks = (N + CHUNK - 1) // CHUNK
    padded = np.zeros((blocks * CHUNK, K), np.float64)
    padded[:N] = terms
    padded = padded.reshape(blocks, PER_THREAD, THREADS, K)
    partials = np.zeros((blocks, K), np.float64)
    for b in range(blocks):
        acc = np.zeros((THREADS, K), np.float64)
        for k in range(PER_THREAD):
            acc = acc + padded[b, k]
        partials[b] = block_reduce(acc)
    rounds = (blocks + THREADS - 1) // THREADS
    padded = np.zeros((rounds * THREADS, K), np.float64)
    padded[:blocks] = partials
    acc = np.zeros((THREADS, K), np.float64)
    for r in range(rounds):
        acc = acc + padded[r * THREADS:(r + 1) * THREADS]
    return block_reduce(acc)


def icp_step(source, T, target, origin, max_dist):
    """-> dict(n, sums [17] f64, idx [N] int32, d2 [N] f64, keep [N] bool)"""
    s = np.asarray(source, np.float64).reshape(-1, 3)
    t = np.asarray(target, np.float64).reshape(-1, 3)
    o = np.asarray(origin, np.float64).reshape(3)
    N = s.shape[0]
    p = transform(T, s)
    with np.errstate(invalid="ignore", over="ignore"):
        _, idx = nn_statement.nn_dist2((p - o).astype(np.float32), (t - o).astype(np.float32))
        has = idx >= 0
        q = np.zeros((N, 3), np.float64)
        q[has] = t[idx[has]]
        dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
        d2 = np.where(has, (dx * dx + dy * dy) + dz * dz, np.inf)
        keep = has & (d2 < np.float64(max_dist) * np.float64(max_dist))
        a, b = p - o, q - o
        cols = [d2, a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]]
        cols += [a[:, i] * b[:, j] for i in range(3) for j in range(3)]
        cols += [(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]]
        terms = np.where(keep[:, None], np.stack(cols, 1), 0.0) if N else np.zeros((0, N_SUMS))
    return {"n": int(keep.sum()), "sums": reduce_terms(terms), "idx": idx.astype(np.int32), "d2": d2, "keep": keep}


def voxel_mean(points, order, heads):
    """segment s = order[heads[s] : heads[s + 1]] (the last to the end): the rows added one by one in that order, then / count"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    order = np.asarray(order)
    ends = list(heads[1:]) + [len(order)]
    out = np.zeros((len(heads), 3), np.float64)
    for s, (b, e) in enumerate(zip(heads, ends)):
        acc = np.zeros(3, np.float64)
        for k in range(int(b), int(e)):
            acc = acc + p[order[k]]
        with np.errstate(invalid="ignore"):
            out[s] = acc / np.float64(int(e) - int(b))
    return out
