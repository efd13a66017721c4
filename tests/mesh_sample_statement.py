"""Numpy statement of gs2m_mesh_sample_count / _emit (include/gs2mesh_amd.h): the DTU evaluation's surface sampler
(evaluation/DTU/eval_code/eval.py:10-19, 48-71) written element-wise in f64 (every numpy operation rounds each element on its own).  tests/test_mesh_sample.py pins it bit for
bit to points the reference's own sample_single_tri returned (tests/golden/dtu_sample_tri.npz) and the kernels to it."""
import numpy as np

MAX_GRID = 1048576
CAP, TOTAL, INDEX = 1, 2, 4


def grid_counts(v0, v1, v2, density):
    """-> (a, b, N1, N2) of one triangle, or None when it gets no grid (area not > 0)"""
    a, b = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        l1 = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        l2 = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        cx = a[1] * b[2] - a[2] * b[1]
        cy = a[2] * b[0] - a[0] * b[2]
        cz = a[0] * b[1] - a[1] * b[0]
        area2 = np.sqrt((cx * cx + cy * cy) + cz * cz)
        if not area2 > 0:
            return None
        thr = np.float64(density) * np.sqrt(l1 * l2 / area2)
        return a, b, np.floor(l1 / thr), np.floor(l2 / thr)


def sample_triangle(v0, v1, v2, density):
    """the samples of one triangle, [n,3] f64, i major and j minor"""
    v0, v1, v2 = (np.asarray(x, np.float64) for x in (v0, v1, v2))
    g = grid_counts(v0, v1, v2, density)
    if g is None or not (g[2] >= 0 and g[3] >= 0):
        return np.zeros((0, 3), np.float64)
    a, b, n1, n2 = g
    c0 = (np.arange(int(n1) + 1, dtype=np.float64) + 0.5) / max(n1, 1e-7)
    c1 = (np.arange(int(n2) + 1, dtype=np.float64) + 0.5) / max(n2, 1e-7)
    i, j = np.nonzero(c0[:, None] + c1[None, :] < 1)          # row-major: i major, j minor
    return (a[None, :] * c0[i, None] + b[None, :] * c1[j, None]) + v0[None, :]


def sample_mesh(vertices, triangles, density):
    """-> (counts [T] u32, offsets [T] u32, points [V + total, 3] f64, status): triangles with an index outside [0, V) or with
    more than MAX_GRID grid nodes get count 0 and set their status bit"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    counts, chunks, status = np.zeros(len(t), np.uint32), [v], 0
    for k, (i0, i1, i2) in enumerate(t):
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= len(v):
            status |= INDEX
            continue
        g = grid_counts(v[i0], v[i1], v[i2], density)
        with np.errstate(over="ignore"):
            capped = g is not None and g[2] >= 0 and g[3] >= 0 and not (g[2] + 1) * (g[3] + 1) <= MAX_GRID
        if capped:
            status |= CAP
            continue
        p = sample_triangle(v[i0], v[i1], v[i2], density)
        counts[k] = len(p)
        chunks.append(p)
    offsets = (np.cumsum(counts, dtype=np.uint64) - counts).astype(np.uint32)
    return counts, offsets, np.concatenate(chunks, 0), status
