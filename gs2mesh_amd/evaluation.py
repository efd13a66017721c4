"""Geometric evaluation of a mesh against a ground-truth point set, on the GPU.

The reference judges its meshes by geometry: DTU accuracy / completeness (evaluation/DTU/eval_code/eval.py), MobileBrick
accuracy / recall / F1 / Chamfer (evaluation/MobileBrick/eval_code/evaluate.py) and the TNT F-score.  The core of all three
is the nearest neighbour of millions of points in another set of millions, which they run on host cores through KD and ball
trees, and (DTU) a surface sampler run in a multiprocessing pool.  Here both are HIP kernels: ``gs2m_nn_dist2`` (exact,
ties to the smallest index) and ``gs2m_mesh_sample_count`` / ``_emit`` (bit-identical to the reference's sampler);
include/gs2mesh_amd.h states their arithmetic.  Everything around them is torch on the same device.

Before it scores a DTU mesh the reference culls it (``cull_scan``, evaluation/DTU/eval_code/evaluate_single_scene.py:21-116):
every view's object mask is dilated with a disk of radius 24 and a vertex survives only if every view sees it outside the
image or on the dilated mask.  That is ``dtu_cull`` here, on two more kernels: ``gs2m_mask_dilate_disk`` (equal to scipy's /
skimage's ``binary_dilation(mask, disk(r))`` bit for bit) and ``gs2m_points_cull_views`` (the reference's f32 projection and
torch's nearest ``grid_sample``, stated operation by operation in the header).  ``dtu_projections`` rebuilds the reference's
``intrinsics @ inverse(pose)`` without cv2 as ``P / ||P[2,:3]||``; equality with cv2's own decomposition was not checked.
``visibility_cull`` is MobileBrick's ``visibility_test`` in torch ops, on the same mesh filter
(``TriangleMesh.remove_vertices_by_mask``).

Precision.  The sampler and every filter work in f64 like the reference.  The nearest-neighbour kernel works in f32, so the
coordinates reach it as ``f32(p - origin)`` with the subtraction in f64; ``origin`` defaults to the midpoint of the ground
truth's bounding box, ``(gt.min(0) + gt.max(0)) / 2``, which keeps the f32 coordinates of a scene of extent E below E / 2
(spacing E * 2^-25: 2e-5 mm on a 600 mm DTU scan).  Distances are ``sqrt`` in f64 of the f32 squared distance, means are f64
sums on the device.

Registration.  MobileBrick and TNT align the prediction to the ground truth with Open3D's ``registration_icp`` before they
score it (evaluation/MobileBrick/eval_code/evaluate.py:82-93; evaluation/TNT/eval_code/python_toolbox/evaluation/run.py:92-124,
registration.py:106-195, evaluation.py:60-88).  ``registration_icp`` is that loop on ``gs2m_icp_prepare`` / ``gs2m_icp_step``
(the target's search structure built once, one kernel pass and one 144-byte copy per iteration) with ``umeyama`` on the host;
``voxel_down_sample`` (``gs2m_voxel_mean``), ``uniform_down_sample`` and ``crop_points`` restate the Open3D calls around it,
``mobilebrick_align``, ``tnt_register`` and ``tnt_evaluate`` the reference's flows.  Open3D's source was not at hand: its keep
rule (strict ``<``), voxel key and polygon test are written as remembered, and say so where they stand.

Outside this module, as in DESIGN.md: TNT's RANSAC trajectory alignment (``init_trans`` is an input; ``umeyama(...,
with_scaling=True)`` on matched camera centres is the stand-in), normals, plots and coloured clouds, Poisson-disk sampling.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import _ptr, _stream_of
from .rasterizer import morton_order

MORTON_MIN_N = 1024     # below this one super-box holds every group: the sort buys nothing


def _torch():
    import torch
    return torch


def _device(device):
    if device is not None:
        return int(device)
    torch = _torch()
    return torch.cuda.current_device() if torch.cuda.is_available() else 0


def _tensor(a, dtype, device=None):
    """anything array-like -> contiguous tensor of ``dtype`` where the memory policy keeps its buffers"""
    torch = _torch()
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.is_cuda:
        return a.to(dtype).contiguous()
    return _lib.MEMORY.upload(a, dtype, _device(device))


def _points(a, dtype, name, device=None):
    t = _tensor(a, dtype, device)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [N,3], got {tuple(t.shape)}")
    return t


# ---- the two kernels ---------------------------------------------------------------------------------------------------

def nearest_neighbors(queries, refs, sort=True, lib=None, want_index=True):
    """``gs2m_nn_dist2``: for every row of ``queries`` [Q,3] f32 the squared distance to, and the index of, its nearest row
    of ``refs`` [R,3] f32 -> (d2 [Q] f32, idx [Q] int32), on the tensors' device, asynchronous on the current stream.
    Exact in the f32 arithmetic of include/gs2mesh_amd.h; exact ties go to the smallest index; R = 0 gives (+inf, -1).
    ``sort``: walk each side of at least 1024 points along its Morton curve (``rasterizer.morton_order``); it changes the
    time, never a bit of the result.  ``want_index=False`` returns (d2, None)."""
    torch = _torch()
    lib = lib or _lib.get()
    q = _points(queries, torch.float32, "queries")
    r = _points(refs, torch.float32, "refs", q.device.index if q.is_cuda else None)
    if r.device != q.device:
        raise ValueError(f"nearest_neighbors: queries on {q.device}, refs on {r.device}")
    Q, R = int(q.shape[0]), int(r.shape[0])
    d2 = torch.empty((Q,), dtype=torch.float32, device=q.device)
    idx = torch.empty((Q,), dtype=torch.int32, device=q.device) if want_index else None
    if Q == 0:
        return d2, idx
    qo = morton_order(q) if sort and Q >= MORTON_MIN_N else None
    ro = morton_order(r) if sort and R >= MORTON_MIN_N else None
    need = int(lib.gs2m_nn_scratch_bytes(Q, R))
    scratch = torch.empty(((need + 15) // 16 * 2,), dtype=torch.int64, device=q.device) if need else None
    _lib.check(lib.gs2m_nn_dist2(Q, _ptr(q, torch.float32, "queries"), _ptr(qo, torch.int32, "query_order"), R,
                                 _ptr(r, torch.float32, "refs"), _ptr(ro, torch.int32, "ref_order"), _ptr(scratch),
                                 0 if scratch is None else scratch.shape[0] * 8, _ptr(d2), _ptr(idx), _stream_of(q, None)), lib)
    return d2, idx


def sample_mesh(mesh_or_arrays, density, lib=None, device=None):
    """The DTU evaluation's mesh -> point set (eval.py:48-71) -> [V + S, 3] f64 on the device: the vertices, then for every
    triangle of non-zero area, in triangle order, its barycentric grid at ``density`` (``gs2m_mesh_sample_count`` /
    ``_emit``, bit-identical to the reference's ``sample_single_tri``).  ``mesh_or_arrays``: a ``mesh.TriangleMesh`` or
    ``(vertices [V,3], triangles [T,3])``.  Raises if a triangle names a vertex outside the mesh, if one triangle would take
    more than 1 048 576 grid nodes or the mesh more than 2^31 - 1 samples (``density`` far too small for the mesh's units),
    and unless 0 < ``density`` < inf (the kernels would give every triangle an empty grid there; the reference fails in
    ``int(n1)``)."""
    torch = _torch()
    if not 0 < float(density) < float("inf"):
        raise ValueError(f"sample_mesh: density must be positive and finite, got {density}")
    lib = lib or _lib.get()
    if hasattr(mesh_or_arrays, "vertices"):
        verts, tris = mesh_or_arrays.vertices, mesh_or_arrays.triangles
    else:
        verts, tris = mesh_or_arrays
    v = _tensor(verts, torch.float64, device).reshape(-1, 3)
    t = _tensor(tris, torch.int32, v.device.index if v.is_cuda else device).reshape(-1, 3)
    V, T = int(v.shape[0]), int(t.shape[0])
    counts = torch.empty((T,), dtype=torch.int32, device=v.device)
    offsets = torch.empty((T,), dtype=torch.int32, device=v.device)
    state = torch.empty((T // 4096 + 4,), dtype=torch.int64, device=v.device)
    total, status = C.c_int64(0), C.c_uint32(0)
    stream = _stream_of(v, None)
    _lib.check(lib.gs2m_mesh_sample_count(V, _ptr(v), T, _ptr(t), float(density), _ptr(counts), _ptr(offsets), _ptr(state),
                                          state.shape[0] * 8, stream, C.byref(total), C.byref(status)), lib)
    if status.value & _lib.MESH_SAMPLE_INDEX:
        raise ValueError(f"sample_mesh: a triangle names a vertex outside 0..{V - 1}")
    if status.value & _lib.MESH_SAMPLE_CAP:
        raise ValueError(f"sample_mesh: a triangle would take more than 1048576 grid nodes at density {density}")
    if status.value & _lib.MESH_SAMPLE_TOTAL:
        raise ValueError(f"sample_mesh: {total.value} samples at density {density}, more than 2^31 - 1")
    points = torch.empty((V + total.value, 3), dtype=torch.float64, device=v.device)
    _lib.check(lib.gs2m_mesh_sample_emit(V, _ptr(v), T, _ptr(t), float(density), _ptr(counts), _ptr(offsets), total.value,
                                         _ptr(points), stream), lib)
    return points


# ---- DTU's cull_scan: disk dilation of the view masks and the per-view vertex cull -------------------------------------------

def dilate_masks(masks, radius, want_bytes=False, lib=None, device=None):
    """``gs2m_mask_dilate_disk``: ``scipy.ndimage.binary_dilation(mask != 0, disk(radius))`` of every mask of ``masks``
    ([n,H,W] u8, array or tensor, or a sequence of [H,W]) -> bits [n,H,nw] int64 on the device, nw = (W + 63) // 64: bit
    ``x & 63`` of word ``x >> 6`` is pixel x, the bits at x >= W are 0 (what ``cull_points`` reads).  ``want_bytes`` adds the
    same as 0 / 1 bytes [n,H,W] u8: -> (bits, bytes).  0 <= radius <= 64; asynchronous on the current stream."""
    torch = _torch()
    lib = lib or _lib.get()
    if not isinstance(masks, (torch.Tensor, np.ndarray)):
        masks = torch.stack(list(masks)) if len(masks) and isinstance(masks[0], torch.Tensor) else np.asarray(masks)
    m = _tensor(masks, torch.uint8, device)
    if m.ndim != 3 or m.shape[1] < 1 or m.shape[2] < 1:
        raise ValueError(f"masks must be [n,H,W] with H, W >= 1, got {tuple(m.shape)}")
    n, H, W = (int(s) for s in m.shape)
    nw = (W + 63) // 64
    bits = torch.empty((n, H, nw), dtype=torch.int64, device=m.device)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=m.device) if want_bytes else None
    need = int(lib.gs2m_mask_dilate_disk_scratch_bytes(n, W, H))
    scratch = torch.empty((max(need, 0) // 8,), dtype=torch.int64, device=m.device)
    ptrs = (C.c_void_p * max(n, 1))(*[m.data_ptr() + i * H * W for i in range(n)])
    _lib.check(lib.gs2m_mask_dilate_disk(n, W, H, ptrs, int(radius), _ptr(bits), _ptr(out), _ptr(scratch), max(need, 0),
                                         _stream_of(m, None)), lib)
    return (bits, out) if want_bytes else bits


def dtu_projections(cameras):
    """The projections ``cull_scan`` builds from a DTU ``cameras.npz`` (evaluate_single_scene.py:29-38, 65-70) ->
    (proj [n,3,4] f32, scale_mat_0 [4,4] f32).  ``cameras``: the dict, or the path of the .npz, of ``world_mat_i`` /
    ``scale_mat_i``, i = 0 .. n - 1.

    The reference takes ``P = (world_mat @ scale_mat)[:3]`` in f32, splits it with ``cv2.decomposeProjectionMatrix`` into
    K, R and the camera centre C, and multiplies ``K / K[2,2] @ [R | -R C]`` back together.  That product is P rescaled so
    that the left 3-vector of its third row has unit length, ``M = P / ||P[2,:3]||``, whenever ``det(P[:,:3]) > 0``; it is
    computed here in f64 and rounded to f32 once.  ``det <= 0`` raises ValueError: which sign cv2 returns there was not
    checked, and no DTU camera is known to be on that side.  The identity was checked against an RQ decomposition
    (scipy); equality with cv2's own output was NOT checked -- cv2 is not a dependency of this package."""
    if isinstance(cameras, (str, bytes)) or hasattr(cameras, "__fspath__"):
        cameras = np.load(cameras)
    n = 0
    while f"world_mat_{n}" in cameras:
        n += 1
    proj = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        P = (np.asarray(cameras[f"world_mat_{i}"]).astype(np.float32) @ np.asarray(cameras[f"scale_mat_{i}"]).astype(np.float32))
        P = P[:3, :4].astype(np.float64)
        if not np.linalg.det(P[:, :3]) > 0:
            raise ValueError(f"dtu_projections: camera {i} has det(P[:, :3]) = {np.linalg.det(P[:, :3])} (must be > 0)")
        proj[i] = (P / np.sqrt((P[2, 0] * P[2, 0] + P[2, 1] * P[2, 1]) + P[2, 2] * P[2, 2])).astype(np.float32)
    scale0 = np.asarray(cameras["scale_mat_0"]).astype(np.float32) if n else np.eye(4, dtype=np.float32)
    return proj, scale0


def cull_points(points, projections, mask_bits, mask_size, norm_size=(1600, 1200), lib=None):
    """``gs2m_points_cull_views`` -> bool [V] on the device: True where point i, in every view, lands outside the image or on
    that view's mask (include/gs2mesh_amd.h states the f32 arithmetic; it is the reference's ``cull_scan`` loop with torch's
    nearest ``grid_sample``).  ``points`` [V,3] f32, ``projections`` [n,3,4] f32 (``dtu_projections``), ``mask_bits``
    [n,H,nw] int64 (``dilate_masks``), ``mask_size`` = (W, H) of the masks, ``norm_size`` = the (W, H) the reference
    normalises pixel coordinates by (it hard-codes DTU's 1600 x 1200)."""
    torch = _torch()
    lib = lib or _lib.get()
    p = _points(points, torch.float32, "points")
    dev = p.device.index if p.is_cuda else None
    proj = _tensor(projections, torch.float32, dev).reshape(-1, 12)
    n = int(proj.shape[0])
    W, H = int(mask_size[0]), int(mask_size[1])
    bits = _tensor(mask_bits, torch.int64, dev)
    if n and tuple(bits.shape) != (n, H, (W + 63) // 64):
        raise ValueError(f"mask_bits must be [{n},{H},{(W + 63) // 64}], got {tuple(bits.shape)}")
    V = int(p.shape[0])
    keep = torch.empty((V,), dtype=torch.uint8, device=p.device)
    _lib.check(lib.gs2m_points_cull_views(V, _ptr(p), n, _ptr(proj), _ptr(bits), W, H, float(norm_size[0]), float(norm_size[1]),
                                          _ptr(keep), _stream_of(p, None)), lib)
    return keep.to(torch.bool)


def _as_mesh(mesh_or_arrays):
    from .mesh import TriangleMesh
    if hasattr(mesh_or_arrays, "vertices"):
        return mesh_or_arrays
    verts, tris = mesh_or_arrays
    t = _torch()
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, t.Tensor) else np.asarray(a)
    return TriangleMesh(host(verts), host(tris))


def _load_mask(m):
    """one view's mask -> [H,W] u8.  A path is read as the reference's ``cv2.imread(p)[:, :, 0]``: the BLUE channel, here
    PIL's ``convert("RGB")`` channel 2; an array [H,W,C] gives its channel 0 (it is taken for cv2's BGR array)."""
    if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
        from PIL import Image
        with Image.open(m) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, 2])
    t = _torch()
    a = m.detach().cpu().numpy() if isinstance(m, t.Tensor) else np.asarray(m)
    if a.ndim == 3:
        a = a[:, :, 0]
    if a.ndim != 2:
        raise ValueError(f"a mask must be [H,W] or [H,W,C], got {a.shape}")
    return np.ascontiguousarray(a != 0).astype(np.uint8)


def dtu_cull(mesh, cameras, masks, radius=24, norm_size=(1600, 1200), lib=None, device=None):
    """The reference's ``cull_scan`` (evaluate_single_scene.py:21-116) -> a new ``TriangleMesh`` in DTU world coordinates:
    every view's mask dilated with ``disk(radius)`` (``dilate_masks``), the vertices (as f32) kept that in every view land
    outside the image or on the dilated mask (``cull_points``), the faces that lost a vertex dropped
    (``remove_vertices_by_mask``), then ``v * scale_mat_0[0,0] + scale_mat_0[:3,3]`` in f64.  ``cameras``: as
    ``dtu_projections``; ``masks``: one per camera, arrays or file paths (``_load_mask``), all of one size."""
    import copy
    torch = _torch()
    mesh = _as_mesh(mesh)
    proj, scale0 = dtu_projections(cameras)
    ms = [_load_mask(m) for m in masks]
    if len(ms) != proj.shape[0]:
        raise ValueError(f"dtu_cull: {len(ms)} masks for {proj.shape[0]} cameras")
    out = copy.deepcopy(mesh)
    if ms:
        if any(m.shape != ms[0].shape for m in ms):
            raise ValueError("dtu_cull: the masks differ in size")
        H, W = ms[0].shape
        bits = dilate_masks(np.stack(ms), radius, lib=lib, device=device)
        verts = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float64)).to(torch.float32)
        keep = cull_points(_tensor(verts, torch.float32, device), proj, bits, (W, H), norm_size, lib=lib)
        out.remove_vertices_by_mask(~keep.cpu().numpy())
    out.vertices = out.vertices * np.float64(scale0[0, 0]) + scale0[:3, 3].astype(np.float64)[None]
    return out


def visibility_cull(mesh, volume, min_pts, resolutions, voxel_size, device=None):
    """MobileBrick's ``visibility_test`` (evaluation/MobileBrick/eval_code/evaluate.py:34-44) as the reference writes it ->
    a new ``TriangleMesh`` without the vertices whose nearest voxel of ``volume`` [D0,D1,D2] is not > 0 (or lies outside
    it), vertex normals recomputed: voxels = (v - min_pts) / voxel_size in f64, scaled to [-1, 1] by ``resolutions - 1``,
    reversed to (z, y, x), cast to f32 and looked up with ``F.grid_sample(mode='nearest', padding_mode='zeros',
    align_corners=True)``.  Torch ops only."""
    import copy
    import torch.nn.functional as F
    torch = _torch()
    mesh = _as_mesh(mesh)
    dev = _lib.MEMORY.buffer_device(_device(device))
    vol = torch.from_numpy(np.ascontiguousarray(volume)).float().to(dev)
    g = (np.asarray(mesh.vertices, np.float64) - np.asarray(min_pts, np.float64)) / voxel_size        # in voxels, f64
    g = g / (np.asarray(resolutions, np.float64) - 1) * 2 - 1                                          # [-1, 1] over the volume
    grid = torch.from_numpy(np.ascontiguousarray(g[:, ::-1])).float().to(dev)                           # (z, y, x): x indexes the last axis
    seen = F.grid_sample(vol[None, None], grid[None, None, None], mode="nearest", padding_mode="zeros", align_corners=True)
    seen = seen[0, 0, 0, 0].cpu().numpy() > 0
    out = copy.deepcopy(mesh)
    out.remove_vertices_by_mask(~seen)
    return out.compute_vertex_normals()


# ---- torch around them -------------------------------------------------------------------------------------------------

def thin_points(points, cell, return_index=False):
    """One point per occupied cubic cell of edge ``cell`` (cell = floor(p / cell) per axis, f64): the point with the lowest
    index wins, and the survivors keep their order.  Torch ops, no kernel.

    This is the deliberate substitute for the reference's thinning (eval.py:79-94), which shuffles the points with an unseeded
    generator and then keeps them greedily -- a point survives unless an earlier survivor lies within ``density`` -- in one
    sequential Python pass: its result differs from run to run of the reference itself, so there is nothing to reproduce.
    Both leave a set whose points are about ``cell`` apart and that covers the input to within ``cell * sqrt(3)``."""
    torch = _torch()
    p = _points(points, torch.float64, "points")
    n = int(p.shape[0])
    if n == 0:
        keep = torch.zeros((0,), dtype=torch.int64, device=p.device)
        return (p, keep) if return_index else p
    if not cell > 0:
        raise ValueError(f"thin_points: cell = {cell}")
    ijk = torch.floor(p / float(cell)).to(torch.int64)
    ijk = ijk - ijk.amin(dim=0)
    dims = (ijk.amax(dim=0) + 1).tolist()
    if dims[0] * dims[1] * dims[2] < 2 ** 62:
        key = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
        _, inv = torch.unique(key, return_inverse=True)
    else:
        _, inv = torch.unique(ijk, dim=0, return_inverse=True)
    first = torch.full((int(inv.max().item()) + 1,), n, dtype=torch.int64, device=p.device)
    first.scatter_reduce_(0, inv, torch.arange(n, dtype=torch.int64, device=p.device), reduce="amin")
    keep = torch.sort(first).values
    return (p[keep], keep) if return_index else p[keep]


def dtu_observation_filter(points, obs_mask, bb, res, patch=60):
    """eval.py:102-110 restated -> (inbound, observed), two bool masks over ``points`` [N,3] f64:
    ``inbound``  = all(p >= f32(BB[0]) - patch) and all(p < f32(BB[1]) + 2 * patch), the bounds in f32 as the reference's;
    ``observed`` = inbound, and g = round_half_even((p - f32(BB[0])) / Res) lies inside ``obs_mask`` and obs_mask[g] is set.
    The reference measures data -> GT on the observed points and GT -> data against the inbound ones."""
    torch = _torch()
    p = _points(points, torch.float64, "points")
    dev = p.device
    bb32 = torch.from_numpy(np.ascontiguousarray(np.asarray(bb, np.float64).reshape(2, 3).astype(np.float32))).to(dev)
    lo = (bb32[0] - float(patch)).to(torch.float64)
    hi = (bb32[1] + float(patch) * 2).to(torch.float64)
    inbound = ((p >= lo) & (p < hi)).all(dim=1)
    mask = torch.from_numpy(np.ascontiguousarray(np.asarray(obs_mask) != 0)).to(dev)
    if mask.ndim != 3:
        raise ValueError(f"obs_mask must be 3-D, got {tuple(mask.shape)}")
    r = float(np.asarray(res, np.float64).reshape(-1)[0])
    g = torch.round((p - bb32[0].to(torch.float64)) / r)
    shape = torch.tensor(list(mask.shape), dtype=torch.float64, device=dev)
    inside = inbound & ((g >= 0) & (g < shape)).all(dim=1)
    gi = torch.where(inside[:, None], g, torch.zeros_like(g)).to(torch.int64)
    observed = inside & mask[gi[:, 0], gi[:, 1], gi[:, 2]]
    return inbound, observed


def above_plane(points, plane):
    """eval.py:128-130 restated -> bool mask: ((P0 * x + P1 * y) + P2 * z) + P3 > 0 in f64."""
    torch = _torch()
    p = _points(points, torch.float64, "points")
    P = [float(x) for x in np.asarray(plane, np.float64).reshape(4)]
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


def _origin(gt, origin):
    torch = _torch()
    if origin is not None:
        return torch.as_tensor(np.asarray(origin, np.float64).reshape(3)).to(gt.device)
    if gt.shape[0] == 0:
        return torch.zeros(3, dtype=torch.float64, device=gt.device)
    return (gt.amin(dim=0) + gt.amax(dim=0)) / 2


def _distances(queries, refs, origin, sort, lib):
    """[Q] f64: sqrt in f64 of the f32 squared distance between f32(queries - origin) and f32(refs - origin)"""
    torch = _torch()
    d2, _ = nearest_neighbors((queries - origin).to(torch.float32), (refs - origin).to(torch.float32), sort=sort, lib=lib,
                              want_index=False)
    return torch.sqrt(d2.to(torch.float64))


def _mean(x):
    return float(x.sum(dtype=_torch().float64).item()) / int(x.shape[0]) if int(x.shape[0]) else float("nan")


def dtu_metrics(pred_points, gt_points, max_dist=20, pred_refs=None, gt_queries=None, origin=None, sort=True, lib=None):
    """eval.py:117-134, 157 -> {mean_d2s, mean_s2d, overall}: ``mean_d2s`` the mean distance from ``pred_points`` to
    ``gt_points``, ``mean_s2d`` from ``gt_queries`` (default: ``gt_points``; the reference: the part above the ground
    plane) to ``pred_refs`` (default: ``pred_points``; the reference: the inbound points before the observation mask), each
    over the distances < ``max_dist`` only (a distance equal to it is left out; none left gives NaN, as numpy's mean of
    nothing), ``overall`` their mean."""
    torch = _torch()
    pred = _points(pred_points, torch.float64, "pred_points")
    dev = pred.device.index if pred.is_cuda else None
    gt = _points(gt_points, torch.float64, "gt_points", dev)
    refs = pred if pred_refs is None else _points(pred_refs, torch.float64, "pred_refs", dev)
    gq = gt if gt_queries is None else _points(gt_queries, torch.float64, "gt_queries", dev)
    o = _origin(gt, origin)
    d2s = _distances(pred, gt, o, sort, lib)
    s2d = _distances(gq, refs, o, sort, lib)
    mean_d2s = _mean(d2s[d2s < max_dist])
    mean_s2d = _mean(s2d[s2d < max_dist])
    return {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2}


def fscore_metrics(pred_points, gt_points, thresholds, origin=None, sort=True, lib=None):
    """MobileBrick's ``evaluate`` (evaluate.py:46-63) for any number of thresholds -> {pred_gt, gt_pred, chamfer,
    thresholds: {str(t): {accuracy, recall, F1}}}: ``pred_gt`` / ``gt_pred`` the mean nearest-neighbour distances,
    ``chamfer`` their sum, ``accuracy`` / ``recall`` the shares of those distances < t, ``F1`` their harmonic mean --
    reported as 0 where both are 0 (the reference divides 0 by 0 there)."""
    torch = _torch()
    pred = _points(pred_points, torch.float64, "pred_points")
    gt = _points(gt_points, torch.float64, "gt_points", pred.device.index if pred.is_cuda else None)
    o = _origin(gt, origin)
    d_pg = _distances(pred, gt, o, sort, lib)
    d_gp = _distances(gt, pred, o, sort, lib)
    out = {"pred_gt": _mean(d_pg), "gt_pred": _mean(d_gp)}
    out["chamfer"] = out["pred_gt"] + out["gt_pred"]
    out["thresholds"] = {}
    for t in thresholds:
        acc = float((d_pg < t).sum().item()) / int(d_pg.shape[0]) if int(d_pg.shape[0]) else float("nan")
        rec = float((d_gp < t).sum().item()) / int(d_gp.shape[0]) if int(d_gp.shape[0]) else float("nan")
        f1 = 0.0 if acc + rec == 0 else 2 * acc * rec / (acc + rec)
        out["thresholds"][str(t)] = {"accuracy": acc, "recall": rec, "F1": f1}
    return out


def evaluate_mesh(mesh, gt_points, density=0.2, max_dist=20, thresholds=(), obs_mask=None, bb=None, res=None, plane=None,
                  patch=60, origin=None, sort=True, lib=None, device=None, cull=None):
    """The DTU evaluation of a mesh (eval.py:43-134), from arrays instead of the dataset's directory: sample at ``density``,
    thin to one point per cell of edge ``density`` (``thin_points``), then -- when ``obs_mask`` / ``bb`` / ``res`` are given --
    keep the inbound and observed points, and -- when ``plane`` is given -- the ground truth above it; ``dtu_metrics`` of what
    is left.  With ``thresholds`` the MobileBrick figures of the same two sets (``fscore_metrics``) come under "fscore".
    With ``cull`` = dict(cameras=..., masks=...[, radius, norm_size]) the mesh first goes through ``dtu_cull``, as the
    reference's run_and_evaluate_dtu.py has it, and "n_vertices_culled" is added.
    -> {mean_d2s, mean_s2d, overall, n_sampled, n_thinned, n_observed, n_gt[, fscore][, n_vertices_culled]}."""
    torch = _torch()
    n_culled = None
    if cull is not None:
        before = _as_mesh(mesh)
        mesh = dtu_cull(before, lib=lib, device=device, **cull)
        n_culled = int(before.vertices.shape[0]) - int(mesh.vertices.shape[0])
    pts = sample_mesh(mesh, density, lib=lib, device=device)
    dev = pts.device.index if pts.is_cuda else None
    gt = _points(gt_points, torch.float64, "gt_points", dev)
    down = thin_points(pts, density)
    data_in, data_obs = down, down
    if obs_mask is not None:
        inbound, observed = dtu_observation_filter(down, obs_mask, bb, res, patch)
        data_in, data_obs = down[inbound], down[observed]
    gt_q = gt if plane is None else gt[above_plane(gt, plane)]
    o = _origin(gt, origin)
    out = dtu_metrics(data_obs, gt, max_dist, pred_refs=data_in, gt_queries=gt_q, origin=o.cpu().numpy(), sort=sort, lib=lib)
    out.update(n_sampled=int(pts.shape[0]), n_thinned=int(down.shape[0]), n_observed=int(data_obs.shape[0]), n_gt=int(gt_q.shape[0]))
    if len(thresholds):
        out["fscore"] = fscore_metrics(data_obs, gt_q, thresholds, origin=o.cpu().numpy(), sort=sort, lib=lib)
    if n_culled is not None:
        out["n_vertices_culled"] = n_culled
    return out


# ---- registration: Umeyama, the ICP loop, and the Open3D calls around it ---------------------------------------------------

class RegistrationResult:
    """What Open3D's ``RegistrationResult`` holds, plus the number of updates made."""

    def __init__(self, transformation, fitness, inlier_rmse, n_iterations, correspondence_set=None):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.n_iterations = n_iterations
        self.correspondence_set = correspondence_set

    def __repr__(self):
        return f"RegistrationResult(fitness={self.fitness:.6g}, inlier_rmse={self.inlier_rmse:.6g}, n_iterations={self.n_iterations})"


def _umeyama_solve(cov, mu_s, mu_d, var_s, with_scaling):
    """Eigen's ``umeyama`` from the centred covariance (1/n) sum (d - mu_d)(s - mu_s)^T, the means and the source variance"""
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = float((D * S).sum() / var_s) if with_scaling and var_s > 0 else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_d - c * (R @ mu_s)
    return T


def umeyama(src, dst, with_scaling=False):
    """The least-squares similarity (or rigid) transform dst ~ c R src + t of matched rows -> 4 x 4 f64, numpy on the host, in
    Eigen's formulation (``Eigen::umeyama``, which Open3D's ``TransformationEstimationPointToPoint`` calls): centred covariance
    ``Sigma = (1/n) sum (d - mu_d)(s - mu_s)^T = U D V^T``, ``S = diag(1, 1, sign(det U det V))``, ``R = U S V^T``,
    ``c = tr(D S) / sigma_s^2`` (1 without scaling), ``t = mu_d - c R mu_s``.  No rows give the identity."""
    s = np.asarray(src, np.float64).reshape(-1, 3)
    d = np.asarray(dst, np.float64).reshape(-1, 3)
    if s.shape != d.shape:
        raise ValueError(f"umeyama: {s.shape[0]} source rows, {d.shape[0]} destination rows")
    n = s.shape[0]
    if n == 0:
        return np.eye(4)
    mu_s, mu_d = s.mean(axis=0), d.mean(axis=0)
    sc, dc = s - mu_s, d - mu_d
    return _umeyama_solve(dc.T @ sc / n, mu_s, mu_d, float((sc * sc).sum() / n), with_scaling)


def umeyama_from_moments(n, sum_p, sum_q, sum_pq, sum_pp, origin=(0.0, 0.0, 0.0), with_scaling=False):
    """``umeyama`` from the sums of ``gs2m_icp_step`` over its n kept pairs: ``sum_p`` = sum p', ``sum_q`` = sum q',
    ``sum_pq[a][b]`` = sum p'_a q'_b, ``sum_pp`` = sum |p'|^2, with p' = p - origin and q' = q - origin.  The covariance is
    ``sum_pq^T / n - mu_q mu_p^T`` and the variance ``sum_pp / n - |mu_p|^2``: raw moments, which cancel like (extent of the
    shifted coordinates / spread of the pairs)^2 -- the reason the kernel shifts by an origin inside the scene.  n = 0 gives the
    identity."""
    n = int(n)
    if n == 0:
        return np.eye(4)
    o = np.asarray(origin, np.float64).reshape(3)
    mu_s = np.asarray(sum_p, np.float64).reshape(3) / n
    mu_d = np.asarray(sum_q, np.float64).reshape(3) / n
    cov = np.asarray(sum_pq, np.float64).reshape(3, 3).T / n - np.outer(mu_d, mu_s)
    var_s = float(sum_pp) / n - float(mu_s @ mu_s)
    T = _umeyama_solve(cov, mu_s, mu_d, var_s, with_scaling)
    T[:3, 3] = (T[:3, 3] + o) - T[:3, :3] @ o                        # from the shifted frame back to the caller's
    return T


def icp_loop(step, n_source, init=None, with_scaling=False, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
             origin=(0.0, 0.0, 0.0)):
    """Open3D's ``RegistrationICP`` loop over ``step(T) -> (n, sums [17] f64)`` (the slots 1..17 of ``gs2m_icp_step``):
    evaluate at ``init``; up to ``max_iteration`` times ``T = umeyama(pairs) @ T`` and evaluate again; stop once
    ``|d fitness| < relative_fitness`` and ``|d rmse| < relative_rmse``.  ``fitness = n / n_source`` (0 for no source),
    ``inlier_rmse = sqrt(sum d2 / n)``, 0 when n = 0.  -> (T, fitness, inlier_rmse, n_iterations).  ``registration_icp`` runs
    it on the kernel; the tests run the same function on the numpy statement of the kernel."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)

    def evaluate(T):
        n, sums = step(T)
        n = int(n)
        return n, sums, (n / n_source if n_source else 0.0), (float(np.sqrt(sums[0] / n)) if n else 0.0)

    n, sums, fitness, rmse = evaluate(T)
    done = 0
    for _ in range(int(max_iteration)):
        update = umeyama_from_moments(n, sums[1:4], sums[4:7], sums[7:16], sums[16], origin, with_scaling)
        T = update @ T
        done += 1
        before = (fitness, rmse)
        n, sums, fitness, rmse = evaluate(T)
        if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
            break
    return T, fitness, rmse, done


def registration_icp(source, target, max_correspondence_distance, init=None, with_scaling=False, relative_fitness=1e-6,
                     relative_rmse=1e-6, max_iteration=30, origin=None, sort=True, want_correspondences=False, lib=None,
                     device=None):
    """Open3D's point-to-point ``registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPoint(with_scaling), ICPConvergenceCriteria(relative_fitness, relative_rmse,
    max_iteration))`` -> ``RegistrationResult`` (``transformation`` 4 x 4 f64 numpy).  The loop is ``icp_loop``; an iteration
    is one ``gs2m_icp_step`` (include/gs2mesh_amd.h: f64 transform, the exact f32 nearest neighbour of ``gs2m_nn_dist2``, the
    f64 keep rule d2 < max^2, fixed-order f64 sums) and one copy of 144 bytes to the host; the target's search structure is
    built once (``gs2m_icp_prepare``).

    Differences from Open3D, on purpose: the kernel applies the accumulated ``T`` to the ORIGINAL source every iteration (Open3D
    transforms its copy in place by every update, so its rounding compounds); the neighbour is the nearest in f32 coordinates
    relative to ``origin`` (default: the midpoint of the target's box), so among targets closer together than f32 resolves
    another one than Open3D's may pair -- its distance and the moments are still f64 of the f64 points.
    ``want_correspondences`` adds ``correspondence_set`` [n,2] int64 (source index, target index) of the last evaluation.
    ``sort``: Morton orders for both sides from 1024 points (the source's at ``init``); the speed only."""
    torch = _torch()
    lib = lib or _lib.get()
    if not 0 < float(max_correspondence_distance) < float("inf"):
        raise ValueError(f"registration_icp: max_correspondence_distance = {max_correspondence_distance}")
    src = _points(source, torch.float64, "source", device)
    tgt = _points(target, torch.float64, "target", src.device.index if src.is_cuda else device)
    if tgt.device != src.device:
        raise ValueError(f"registration_icp: source on {src.device}, target on {tgt.device}")
    N, R = int(src.shape[0]), int(tgt.shape[0])
    T0 = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    o_t = _origin(tgt, origin)
    o = np.ascontiguousarray(o_t.detach().cpu().numpy(), np.float64)
    ro = morton_order((tgt - o_t).to(torch.float32)) if sort and R >= MORTON_MIN_N else None
    qo = None
    if sort and N >= MORTON_MIN_N:
        M = torch.from_numpy(T0).to(src.device)
        moved = src @ M[:3, :3].T + M[:3, 3] - o_t
        qo = morton_order(torch.nan_to_num(moved).to(torch.float32))
    need = int(lib.gs2m_icp_scratch_bytes(N, R))
    scratch = torch.empty(((need + 15) // 16 * 2,), dtype=torch.int64, device=src.device) if need else None
    nbytes = 0 if scratch is None else scratch.shape[0] * 8
    sums = torch.zeros((_lib.ICP_SUMS,), dtype=torch.int64, device=src.device)
    idx = torch.empty((N,), dtype=torch.int32, device=src.device) if want_correspondences else None
    d2 = torch.empty((N,), dtype=torch.float64, device=src.device) if want_correspondences else None
    stream = _stream_of(src, None)
    o_ptr = o.ctypes.data_as(C.c_void_p)
    _lib.check(lib.gs2m_icp_prepare(R, _ptr(tgt), o_ptr, _ptr(ro, torch.int32, "ref_order"), _ptr(scratch), nbytes, stream), lib)

    def step(T):
        Th = np.ascontiguousarray(T, np.float64)
        _lib.check(lib.gs2m_icp_step(N, _ptr(src), _ptr(qo, torch.int32, "query_order"), Th.ctypes.data_as(C.c_void_p), R, _ptr(tgt),
                                     o_ptr, float(max_correspondence_distance), _ptr(scratch), nbytes, _ptr(sums), _ptr(idx),
                                     _ptr(d2), stream), lib)
        host = sums.cpu().numpy()                                     # the iteration's one copy; it waits for the step
        return int(host[0]), host[1:].copy().view(np.float64)

    T, fitness, rmse, done = icp_loop(step, N, T0, with_scaling, relative_fitness, relative_rmse, max_iteration, o)
    pairs = None
    if want_correspondences:
        kept = (idx >= 0) & (d2 < float(max_correspondence_distance) * float(max_correspondence_distance))
        i = torch.nonzero(kept).reshape(-1)
        pairs = torch.stack([i, idx[i].to(torch.int64)], dim=1).cpu().numpy()
    return RegistrationResult(T, fitness, rmse, done, pairs)


def voxel_down_sample(points, voxel_size, lib=None):
    """Open3D's ``PointCloud.voxel_down_sample`` for points alone -> [S,3] f64 on the points' device: voxel
    ``floor((p - (min - voxel_size / 2)) / voxel_size)`` per axis in f64 (Open3D's key, as remembered), every occupied voxel's
    mean with the rows added in ascending original index (``gs2m_voxel_mean``: the order of Open3D's ``AccumulatedPoint``,
    so the means carry its bits).  The output is in ascending (i, j, k) of the voxel; Open3D's is the iteration order of an
    ``unordered_map``, so there is no order to reproduce."""
    torch = _torch()
    lib = lib or _lib.get()
    p = _points(points, torch.float64, "points")
    n = int(p.shape[0])
    if not float(voxel_size) > 0:
        raise ValueError(f"voxel_down_sample: voxel_size = {voxel_size}")
    if n == 0:
        return p
    if n > 2 ** 31 - 1:
        raise ValueError(f"voxel_down_sample: {n} points, more than 2^31 - 1")
    lo = p.amin(dim=0) - float(voxel_size) * 0.5
    ijk = torch.floor((p - lo) / float(voxel_size)).to(torch.int64)
    dims = (ijk.amax(dim=0) + 1).tolist()
    if dims[0] * dims[1] * dims[2] < 2 ** 62:
        key = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    else:
        _, key = torch.unique(ijk, dim=0, return_inverse=True)           # rows sort lexicographically: the same order
    key, order = torch.sort(key, stable=True)
    head = torch.ones((n,), dtype=torch.bool, device=p.device)
    head[1:] = key[1:] != key[:-1]
    heads = torch.nonzero(head).reshape(-1).to(torch.int32).contiguous()
    order = order.to(torch.int32).contiguous()
    S = int(heads.shape[0])
    means = torch.empty((S, 3), dtype=torch.float64, device=p.device)
    _lib.check(lib.gs2m_voxel_mean(n, _ptr(p), _ptr(order), S, _ptr(heads), _ptr(means), _stream_of(p, None)), lib)
    return means


def uniform_down_sample(points, every_k):
    """Open3D's ``uniform_down_sample``: the rows 0, k, 2k, ..."""
    if int(every_k) < 1:
        raise ValueError(f"uniform_down_sample: every_k = {every_k}")
    return _points(points, _torch().float64, "points")[::int(every_k)].contiguous()


def read_crop_volume(json_path):
    """A ``SelectionPolygonVolume`` file (TNT's ``<scene>.json``) -> dict(orthogonal_axis "x" / "y" / "z", axis_min, axis_max,
    bounding_polygon [M,3] f64)."""
    import json
    with open(json_path) as f:
        d = json.load(f)
    axis = str(d["orthogonal_axis"]).lower()
    if axis not in ("x", "y", "z"):
        raise ValueError(f"read_crop_volume: orthogonal_axis = {d['orthogonal_axis']!r}")
    return {"orthogonal_axis": axis, "axis_min": float(d["axis_min"]), "axis_max": float(d["axis_max"]),
            "bounding_polygon": np.asarray(d["bounding_polygon"], np.float64).reshape(-1, 3)}


def crop_points(points, volume, return_mask=False):
    """Open3D's ``SelectionPolygonVolume.crop_point_cloud`` for points alone, as remembered (``CropInPolygon``): with w the
    orthogonal axis and (u, v) the other two in ascending order, a point stays iff ``axis_min <= p_w <= axis_max`` (both ends
    inclusive) and the even-odd rule puts (p_u, p_v) inside ``bounding_polygon``: every edge (a, b) with
    ``(p_v < a_v) != (p_v < b_v)`` is crossed at ``a_u + (p_v - a_v) / (b_v - a_v) * (b_u - a_u)``, and the point is inside
    iff an odd number of crossings lie at u < p_u.  Torch ops, no kernel.  -> the kept rows, in order (or the bool mask)."""
    torch = _torch()
    p = _points(points, torch.float64, "points")
    w = "xyz".index(str(volume["orthogonal_axis"]).lower())
    u, v = [a for a in range(3) if a != w]
    poly = np.asarray(volume["bounding_polygon"], np.float64).reshape(-1, 3)
    keep = (p[:, w] >= float(volume["axis_min"])) & (p[:, w] <= float(volume["axis_max"]))
    inside = torch.zeros_like(keep)
    pu, pv = p[:, u], p[:, v]
    for i in range(poly.shape[0]):
        a, b = poly[i], poly[(i + 1) % poly.shape[0]]
        if a[v] == b[v]:
            continue                                                  # never crossed: (p_v < a_v) == (p_v < b_v)
        crossed = (pv < float(a[v])) != (pv < float(b[v]))
        node = float(a[u]) + (pv - float(a[v])) / float(b[v] - a[v]) * float(b[u] - a[u])
        inside = inside ^ (crossed & (node < pu))
    keep = keep & inside
    return keep if return_mask else p[keep]


def _apply(T, points):
    torch = _torch()
    M = torch.from_numpy(np.ascontiguousarray(T, np.float64).reshape(4, 4)).to(points.device)
    return points @ M[:3, :3].T + M[:3, 3]


def mobilebrick_align(pred_mesh, gt_mesh, threshold=0.02, max_iteration=10, min_fitness=0.99, lib=None, device=None):
    """MobileBrick's alignment (evaluate.py:82-93) -> (mesh, result): ``registration_icp`` with the GT vertices as the source
    and the predicted vertices as the target, rigid, from the identity; a copy of ``pred_mesh`` transformed by
    ``inv(result.transformation)`` when ``result.fitness > min_fitness``, an untouched copy otherwise, as the reference has it."""
    import copy
    pred, gt = _as_mesh(pred_mesh), _as_mesh(gt_mesh)
    result = registration_icp(gt.vertices, pred.vertices, threshold, max_iteration=max_iteration, lib=lib, device=device)
    out = copy.deepcopy(pred)
    if result.fitness > min_fitness:
        out.transform(np.linalg.inv(result.transformation))
    return out, result


TNT_MAX_POINTS = 4e6        # registration.py:41


def tnt_register(pred_points, gt_points, init_trans, crop_volume, tau, lib=None, device=None):
    """TNT's three refinement stages (run.py:98-102, registration.py:106-195) -> (transformation 4 x 4, [the three results]).
    Each stage moves the prediction by the transform so far, crops both clouds with ``crop_volume``, thins them, runs
    ``registration_icp`` with scaling from the identity (relative criteria 1e-6, 20 iterations) and multiplies the result on:
    voxel tau / threshold 80 tau, voxel tau / 2 / threshold 20 tau, then every k-th point with k = round(n / 4e6) where a
    cloud has more than 4e6 points / threshold 2 tau.  ``init_trans`` is the reference's trajectory alignment, an input here."""
    torch = _torch()
    pred = _points(pred_points, torch.float64, "pred_points", device)
    gt = _points(gt_points, torch.float64, "gt_points", pred.device.index if pred.is_cuda else device)
    T = np.array(init_trans, np.float64).reshape(4, 4)
    tau = float(tau)
    gt_crop = crop_points(gt, crop_volume)

    def thin(p, voxel):
        if voxel is not None:
            return voxel_down_sample(p, voxel, lib=lib)
        n = int(p.shape[0])
        return uniform_down_sample(p, int(round(n / TNT_MAX_POINTS))) if n > TNT_MAX_POINTS else p

    results = []
    for voxel, threshold in ((tau, 80 * tau), (tau / 2.0, 20 * tau), (None, 2 * tau)):
        s = thin(crop_points(_apply(T, pred), crop_volume), voxel)
        t = thin(gt_crop, voxel)
        r = registration_icp(s, t, threshold, with_scaling=True, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=20,
                             lib=lib)
        T = r.transformation @ T
        results.append(r)
    return T, results


def tnt_evaluate(pred_points, gt_points, init_trans, crop_volume, tau, sort=True, lib=None, device=None):
    """TNT's evaluation of a point cloud (run.py:92-124, evaluation.py:60-88, 173-177): ``tnt_register``, then both clouds
    cropped and voxel-down-sampled at tau / 2, ``precision`` = the share of prediction -> GT distances < tau, ``recall`` = the
    share of GT -> prediction distances < tau, ``fscore`` their harmonic mean (0 where both are 0).  The distances go through
    ``_distances`` like every other metric here.  -> {precision, recall, fscore, transformation, n_source, n_target}."""
    torch = _torch()
    pred = _points(pred_points, torch.float64, "pred_points", device)
    gt = _points(gt_points, torch.float64, "gt_points", pred.device.index if pred.is_cuda else device)
    tau = float(tau)
    T, _ = tnt_register(pred, gt, init_trans, crop_volume, tau, lib=lib, device=device)
    s = voxel_down_sample(crop_points(_apply(T, pred), crop_volume), tau / 2.0, lib=lib)
    t = voxel_down_sample(crop_points(gt, crop_volume), tau / 2.0, lib=lib)
    o = _origin(t, None)
    share = lambda d: float((d < tau).sum().item()) / int(d.shape[0]) if int(d.shape[0]) else float("nan")
    precision, recall = share(_distances(s, t, o, sort, lib)), share(_distances(t, s, o, sort, lib))
    fscore = 0.0 if precision + recall == 0 else 2 * recall * precision / (recall + precision)
    return {"precision": precision, "recall": recall, "fscore": fscore, "transformation": T, "n_source": int(s.shape[0]),
            "n_target": int(t.shape[0])}
