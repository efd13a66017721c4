"""Plain numpy statement of gs2m_knn_mean_dist2 (include/gs2mesh_amd.h): brute force in float32, chunked.
d = (dx*dx + dy*dy) + dz*dz with every operation rounded to f32; self excluded by index; a d that is NaN or not below
FLT_MAX never counts (a NaN or infinite coordinate, a distance that overflows): it is a neighbour at "no distance" and
stands as FLT_MAX, like a missing one; the three smallest padded with FLT_MAX; out = ((b0 + b1) + b2) / float32(3).
So a point with a NaN or infinite coordinate gets +inf and changes no other point's result."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def mean_dist2(points, chunk=256):
    p = np.ascontiguousarray(points, np.float32)
    P = p.shape[0]
    out = np.empty(P, np.float32)
    three = np.float32(3)
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, P, chunk):
            q = p[i0:i0 + chunk]
            dx = p[None, :, 0] - q[:, None, 0]
            dy = p[None, :, 1] - q[:, None, 1]
            dz = p[None, :, 2] - q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            d[~(d < FLT_MAX)] = FLT_MAX                                             # NaN, +inf: never counts
            d[np.arange(q.shape[0]), np.arange(i0, i0 + q.shape[0])] = FLT_MAX      # self, by index
            if P < 4:
                d = np.concatenate([d, np.full((q.shape[0], 4 - P), FLT_MAX, np.float32)], axis=1)
            b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            out[i0:i0 + chunk] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / three
    return out
