"""``distCUDA2`` of the reference's ``simple_knn._C`` (submodules/simple-knn/spatial.cu:15-26): for every point the mean
squared distance to its three nearest neighbours, computed by ``gs2m_knn_mean_dist2`` (include/gs2mesh_amd.h states the
arithmetic; the result is the exact 3-NN).  The Morton sort the reference runs inside the call with a library radix sort
(simple_knn.cu:185-213) is preparation done with torch (``rasterizer.morton_order``) and only affects the speed."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .._lib import _empty, _is_torch, _ptr, _stream_of
from ..rasterizer import morton_order

MORTON_MIN_P = 1024     # below this one super-box holds every group: the sort buys nothing


def knn_mean_dist2(points, order=None, lib=None, stream=None):
    """``gs2m_knn_mean_dist2`` on a contiguous [P,3] f32 device tensor (numpy array on the emulator back-end of the tests).
    ``order``: None, or an int32 permutation [P] in which the kernel walks the points.  -> [P] f32, asynchronous on the
    stream; the scratch is kept per device and only grows."""
    lib = lib or _lib.get()
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"knn_mean_dist2: points must be [P,3], got {tuple(points.shape)}")
    P = int(points.shape[0])
    if order is not None and tuple(order.shape) != (P,):
        raise ValueError(f"knn_mean_dist2: order must be [{P}], got {tuple(order.shape)}")
    out = _empty(points, (P,), np.float32)
    if P == 0:
        return out
    need = int(lib.gs2m_knn_scratch_bytes(P))
    scratch = _lib.scratch("knn", points, need)
    f32 = i32 = None
    if _is_torch(points):
        import torch
        f32, i32 = torch.float32, torch.int32
    elif points.dtype != np.float32 or (order is not None and order.dtype != np.int32):
        raise TypeError("knn_mean_dist2: points must be float32 and order int32")
    _lib.check(lib.gs2m_knn_mean_dist2(P, _ptr(points, f32, "points"), _ptr(order, i32, "order"), _ptr(scratch),
                                       scratch.shape[0] * 8, _ptr(out), _stream_of(points, stream)), lib)
    return out


def distCUDA2(points):
    """[P,3] float tensor on a HIP device -> [P] float32 on that device."""
    import torch
    if not isinstance(points, torch.Tensor):
        raise RuntimeError(f"distCUDA2 takes a torch tensor on a HIP device, got {type(points).__name__}")
    pts = points.detach().to(torch.float32).contiguous()
    _ptr(pts, torch.float32, "points")      # a CPU tensor is an error (the memory policy of _lib), before any work
    order = morton_order(pts) if pts.shape[0] >= MORTON_MIN_P else None
    return knn_mean_dist2(pts, order)
