"""Plain numpy statement of gs2m_nn_dist2 (include/gs2mesh_amd.h): brute force in float32, chunked.
d = (dx*dx + dy*dy) + dz*dz with every operation rounded to f32; the best starts at (+inf, none) and candidate j replaces it
when d < best, or d == best and j is the smaller index (none is larger than every index); a NaN d never replaces."""
import numpy as np


def nn_dist2(queries, refs, chunk=256):
    """-> (d2 [Q] f32, idx [Q] int32): the argmin by (d, j); -1 where nothing replaced the start"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    r = np.ascontiguousarray(refs, np.float32).reshape(-1, 3)
    Q, R = q.shape[0], r.shape[0]
    out_d = np.full(Q, np.inf, np.float32)
    out_i = np.full(Q, -1, np.int32)
    if R == 0:
        return out_d, out_i
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, Q, chunk):
            c = q[i0:i0 + chunk]
            dx = r[None, :, 0] - c[:, None, 0]
            dy = r[None, :, 1] - c[:, None, 1]
            dz = r[None, :, 2] - c[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            nan = np.isnan(d)
            d[nan] = np.inf                                   # cannot win on d; must not win the index either
            best = d.min(axis=1)
            cand = (d == best[:, None]) & ~nan
            has = cand.any(axis=1)
            j = np.argmax(cand, axis=1)                       # the first True: the smallest index among the ties
            out_d[i0:i0 + chunk] = np.where(has, best, np.float32(np.inf))
            out_i[i0:i0 + chunk] = np.where(has, j, -1)
    return out_d, out_i
