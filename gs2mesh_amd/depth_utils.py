"""Depth without a matcher: ``RenderedDepth`` hands ``TSDF`` the depth map the rasteriser renders from the splat itself.

It plays the role ``Stereo`` plays for ``TSDF`` -- same constructor shape, ``model_name``, ``run``, ``frame_source``, ``close`` and
the same on-disk layout -- but needs no right eye and no matcher.  This is the baseline the GS2Mesh paper argues AGAINST, and
what 2DGS-style meshers fuse: the depth of a pixel is built from the view-space z of the CENTRES of the Gaussians that
contribute to it, which is not the intersection of the pixel's ray with a surface.  The paper's claim is that stereo depth
on rendered pairs beats it; it is here so that the comparison, and a stand-alone run without DLNR weights, can be made.

Per left camera ``run`` does ONE operator-path forward (``gaussian_renderer.render(..., return_depth=True)``), so colour, depth
and opacity come from the same call:
  * ``kind="median"`` (default): z of the contributor that takes the transmittance to one half or below -- a z some Gaussian
    really has, 0 where the accumulated opacity stays under 0.5;
  * ``kind="expected"``: the alpha-weighted mean z of the contributors -- smooth, but between the layers where two overlap;
  * ``kind="ray_median"`` / ``"ray_expected"``: the same two with the depth at which the pixel's ray meets each contributing
    Gaussian in place of its centre's z (``gs2m_rasterize_depth_ray``, one more kernel pair per view): the plane of a flat
    Gaussian instead of a staircase on every surface that is not fronto-parallel -- the baseline the depth-from-splat meshers
    (2DGS, GOF, RaDe-GS) fuse.  Isotropic Gaussians carry no orientation and gain nothing;
  * the occlusion mask of the layout is ``alpha >= alpha_min``: a free foreground mask where no object masker exists.
No gradient flows through any of it.

Depth across views: ``depth_consistency`` is the outlier test between any depth stage (``Stereo``, ``RenderedDepth``, files) and
the TSDF.  Every pixel is lifted with its depth into its view's nearest neighbours (``select_sources``, ``pair_matrices``) and
kept where enough of them see the same surface and few see through it (``gs2m_depth_consistency``; include/gs2mesh_amd.h
states the vote).  ``TSDF(..., consistency=...)`` runs it before the first frame is fused.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _lib
from .stereo_utils import _ViewWriter

KINDS = {"median": "median_depth", "expected": "depth", "ray_median": "ray_median_depth", "ray_expected": "ray_depth"}


def select_sources(camera_to_world, k=4, max_angle_deg=70.0):
    """The source views of every view: int32 [n,k], per view the ``k`` nearest OTHER camera centres among the views whose
    optical axis (+z of the camera) differs from its own by at most ``max_angle_deg``; nearest first, -1 where fewer qualify.
    Computed in f64 on the host.  Ties go to the lower index, and two distances tie when they agree to 1e-9 of the smaller
    one: the neighbours left and right on a ring are equally far on paper, not in f64."""
    E = np.asarray(camera_to_world, np.float64).reshape(-1, 4, 4)
    n, k = E.shape[0], int(k)
    if k < 0 or k > _lib.CONSISTENCY_MAX_SOURCES:
        raise ValueError(f"select_sources: k must be in 0 .. {_lib.CONSISTENCY_MAX_SOURCES}, got {k}")
    centre = E[:, :3, 3]
    axis = E[:, :3, 2] / np.linalg.norm(E[:, :3, 2], axis=1, keepdims=True)
    out = np.full((n, k), -1, np.int32)
    for i in range(n):
        dist = np.linalg.norm(centre - centre[i], axis=1)
        angle = np.degrees(np.arccos(np.clip(axis @ axis[i], -1.0, 1.0)))
        left = [j for j in range(n) if j != i and angle[j] <= max_angle_deg]
        for slot in range(min(k, len(left))):
            nearest = min(dist[j] for j in left)
            j = min(j for j in left if dist[j] <= nearest * (1.0 + 1e-9))
            out[i, slot] = j
            left.remove(j)
    return out


def pair_matrices(camera_to_world, sources):
    """float32 [n,k,12]: for view i and its source j = sources[i][k] the row-major 3 x 4 transform from i's camera frame to
    j's, ``(inv(E_j) @ E_i)[:3]`` in f64, rounded to f32 once.  Rows of -1 sources are zero."""
    E = np.asarray(camera_to_world, np.float64).reshape(-1, 4, 4)
    sources = np.asarray(sources, np.int64).reshape(E.shape[0], -1) if E.shape[0] else np.zeros((0, 0), np.int64)
    inv = np.linalg.inv(E) if E.shape[0] else E
    out = np.zeros(sources.shape + (12,), np.float32)
    for i in range(sources.shape[0]):
        for k, j in enumerate(sources[i]):
            if j >= 0:
                out[i, k] = (inv[j] @ E[i])[:3].reshape(12).astype(np.float32)
    return out


@dataclass
class ConsistencyParams:
    """``sources``: how many source views a view votes with (``select_sources`` picks them), or an explicit int [n,k] table
    (-1 = none).  ``rel_tol``: a source supports a pixel when its depth there is within ``rel_tol`` x the pixel's depth in
    the source's frame.  A pixel is kept with at least ``min_support`` supporting sources and at most ``max_violation`` that
    see through it.  ``max_angle_deg``: see ``select_sources``."""
    sources: object = 4
    rel_tol: float = 0.01
    min_support: int = 2
    max_violation: int = 1
    max_angle_deg: float = 70.0

    @classmethod
    def coerce(cls, value):
        """None / False -> None (off); True -> the defaults; a dict of fields; an instance as it is"""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls(**value)
        raise TypeError(f"consistency must be None, True, a dict or a ConsistencyParams, got {type(value).__name__}")


def _intrinsic4(intr):
    if hasattr(intr, "fx"):
        return float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy)
    fx, fy, cx, cy = (float(v) for v in intr)
    return fx, fy, cx, cy


def consistency_votes(depths, intrinsics, sources, pair, rel_tol, min_support, max_violation, masks=None, min_depth=0.0,
                      max_depth=float("inf"), want=("keep",), lib=None, stream=None, device=None):
    """``gs2m_depth_consistency`` as it is: one call over ``depths`` (list of [H,W] f32 device tensors; sizes may differ) with
    the caller's ``sources`` int32 [n,K] and ``pair`` f32 [n,K,12].  ``intrinsics``: per view an object with fx, fy, cx, cy or
    that 4-tuple.  ``masks``: None, or a list of [H,W] masks / None (0 = the pixel has no depth).  ``want`` names the outputs
    out of keep, support, violation, occluded; returns a dict of lists of [H,W] u8 device tensors.  No host synchronisation:
    inputs already on the device are taken as they are (host arrays are uploaded to ``device``, default: where the first depth
    lives, else 0) and the kernels go on ``stream`` (default: torch's current one).  Uploads, conversions and the outputs are
    made on torch's current stream; an explicit ``stream`` (a hipStream_t handle) is made to wait for that stream, and the
    buffers this call created are recorded on it, so that the allocator does not hand them out again before the kernels ran."""
    import torch
    lib = lib if lib is not None else _lib.get()
    mem = _lib.MEMORY
    n = len(depths)
    unknown = set(want) - {"keep", "support", "violation", "occluded"}
    if unknown:
        raise ValueError(f"consistency_votes: unknown outputs {sorted(unknown)}")
    if len(intrinsics) != n or (masks is not None and len(masks) != n):
        raise ValueError("consistency_votes: depths / intrinsics / masks must have the same length")
    sources = np.ascontiguousarray(np.asarray(sources, np.int32).reshape(n, -1)) if n else np.zeros((0, 0), np.int32)
    K = sources.shape[1]
    pair = np.ascontiguousarray(np.asarray(pair, np.float32).reshape(n, K, 12))
    first = depths[0] if n else None
    if device is None:
        device = first.device.index if _lib._is_torch(first) and first.is_cuda else 0
    views = (_lib.DepthView * max(n, 1))()
    held, outs = [], {name: [] for name in want}
    out_p = {name: (C.c_void_p * max(n, 1))() for name in want}
    for i in range(n):
        d = mem.upload(depths[i], torch.float32, device)
        if d.ndim != 2:
            raise ValueError(f"consistency_votes: depth {i} must be [H,W], got {tuple(d.shape)}")
        H, W = int(d.shape[0]), int(d.shape[1])
        m = None
        if masks is not None and masks[i] is not None:
            m = masks[i]
            if _lib._is_torch(m) and m.dtype not in (torch.uint8, torch.bool):
                m = m != 0
            elif not _lib._is_torch(m):
                m = np.asarray(m)
                m = m.view(np.uint8) if m.dtype == np.bool_ else (m if m.dtype == np.uint8 else (m != 0).view(np.uint8))
            m = mem.upload(m, torch.uint8, device)
            if tuple(m.shape) != (H, W):
                raise ValueError(f"consistency_votes: mask {i} is {tuple(m.shape)}, its depth {(H, W)}")
        held += [d, m]
        fx, fy, cx, cy = _intrinsic4(intrinsics[i])
        views[i] = _lib.DepthView(mem.ptr(d), mem.ptr(m), W, H, fx, fy, cx, cy)
        for name in want:
            o = mem.empty((H, W), np.uint8, device)            # the kernel writes every pixel of an output it is given
            outs[name].append(o)
            out_p[name][i] = mem.ptr(o)
    st = C.c_void_p(int(stream)) if stream is not None else mem.current_stream(device)
    ours = [t for t in held + [o for name in want for o in outs[name]] if _lib._is_torch(t) and t.is_cuda]
    if stream is not None and ours:
        ext = torch.cuda.ExternalStream(int(stream), device=ours[0].device)
        ext.wait_stream(torch.cuda.current_stream(ours[0].device))
        for t in ours:                                         # also inputs the caller owns: recording them is harmless
            t.record_stream(ext)
    _lib.check(lib.gs2m_depth_consistency(
        n, views, K, sources.ctypes.data_as(C.POINTER(C.c_int32)), pair.ctypes.data_as(C.POINTER(C.c_float)), float(rel_tol),
        float(min_depth), float(max_depth), int(min_support), int(max_violation), out_p.get("keep"), out_p.get("support"),
        out_p.get("violation"), out_p.get("occluded"), st), lib)
    return outs


def depth_consistency(depths, intrinsics, camera_to_world, params=None, masks=None, min_depth=0.0, max_depth=float("inf"),
                      want_counts=False, lib=None, stream=None, device=None):
    """The keep masks of ``depths`` (list of [H,W] f32 device tensors, one per view) under the poses ``camera_to_world`` [n,4,4]
    and ``params`` (``ConsistencyParams``, a dict of its fields, None / True = the defaults): list of [H,W] u8 device tensors,
    1 = keep.  ``intrinsics``: one per view, or one for all.  ``masks`` / ``min_depth`` / ``max_depth`` say which pixels have a
    depth at all (in the reference view and in a source alike).  With ``want_counts`` returns ``(keep, support, violation,
    occluded)``.  One ``gs2m_depth_consistency`` call; no host synchronisation of its own."""
    params = ConsistencyParams.coerce(True if params is None else params)
    n = len(depths)
    if hasattr(intrinsics, "fx") or (len(intrinsics) == 4 and not hasattr(intrinsics[0], "fx") and np.ndim(intrinsics[0]) == 0):
        intrinsics = [intrinsics] * n
    if np.ndim(params.sources) == 0:
        sources = select_sources(camera_to_world, int(params.sources), params.max_angle_deg)
    else:
        sources = np.asarray(params.sources, np.int32).reshape(n, -1) if n else np.zeros((0, 0), np.int32)
    pair = pair_matrices(camera_to_world, sources)
    want = ("keep", "support", "violation", "occluded") if want_counts else ("keep",)
    out = consistency_votes(depths, intrinsics, sources, pair, params.rel_tol, params.min_support, params.max_violation,
                            masks=masks, min_depth=min_depth, max_depth=max_depth, want=want, lib=lib, stream=stream,
                            device=device)
    return tuple(out[name] for name in want) if want_counts else out["keep"]


class RenderedDepth:
    """``TSDF(renderer, RenderedDepth(base_dir, renderer, args), args, name)`` fuses the written files
    (``<NNN>/left.png``, ``<NNN>/out_RENDER/depth.npy``, ``<NNN>/out_RENDER/occlusion_mask.npy``);
    ``run(keep_on_device=True)`` + ``TSDF(..., frame_source=rd.frame_source)`` hands the maps over in memory, as the dict
    ``Stereo.frame_source`` gives: ``image`` [H,W,3] u8, ``depth`` [H,W] f32, ``occlusion`` [H,W] u8 (0 / 1).
    ``renderer`` needs ``left_cameras``, ``left_view(camera_number)`` and ``render_folder_name(camera_number)``."""

    model_name = "RENDER"

    def __init__(self, base_dir, renderer, args, device="cuda", kind="median", alpha_min=0.5):
        if kind not in KINDS:
            raise ValueError(f"RenderedDepth: kind must be one of {sorted(KINDS)}, got {kind!r}")
        if not 0.0 < float(alpha_min) <= 1.0:
            raise ValueError(f"RenderedDepth: alpha_min must be in (0, 1], got {alpha_min!r}")
        self.base_dir = base_dir
        self.renderer = renderer
        self.args = args
        self.device = device
        self.kind = kind
        self.alpha_min = float(alpha_min)
        self.frames = {}        # keep_on_device: camera number -> dict(image, depth, occlusion)
        self.timings = {}       # host wall seconds of the last run(): render, write_wait, total
        self._writer = None

    def render_view(self, camera_number):
        """one forward of the left camera -> dict(image [H,W,3] u8, depth [H,W] f32, occlusion [H,W] u8), where the model lives"""
        import torch
        from .gaussian_renderer import render
        cam, gaussians, background = self.renderer.left_view(camera_number)
        with torch.no_grad():
            out = render(cam, gaussians, getattr(self.args, "pipe", None), background, return_depth=True,
                         ray_depth=self.kind.startswith("ray_"))
            # the 8-bit image as torchvision's save_image quantises it (the reference's left.png)
            image = out["render"].clamp(0.0, 1.0).mul(255.0).add_(0.5).clamp_(0.0, 255.0).to(torch.uint8)
            image = image.permute(1, 2, 0).contiguous()
            occlusion = (out["alpha"] >= self.alpha_min).to(torch.uint8)
        return dict(image=image, depth=out[KINDS[self.kind]], occlusion=occlusion)

    def frame_source(self, camera_number):
        """for ``TSDF(..., frame_source=rendered.frame_source)`` after ``run(keep_on_device=True)``"""
        try:
            return self.frames[camera_number]
        except KeyError:
            raise RuntimeError(f"RenderedDepth.frame_source: view {camera_number} was not kept "
                               "(run(keep_on_device=True) from a start that covers it)") from None

    def run(self, start=0, keep_on_device=False, write_files=True):
        import time
        tm = self.timings = dict(render=0.0, write_wait=0.0, total=0.0)
        t_run = time.perf_counter()
        if write_files and self._writer is None:
            self._writer = _ViewWriter()
        for camera_number, _ in enumerate(self.renderer.left_cameras):
            if camera_number < start:
                continue
            t0 = time.perf_counter()
            fr = self.render_view(camera_number)
            t1 = time.perf_counter()
            tm["render"] += t1 - t0
            if keep_on_device:
                self.frames[camera_number] = fr
            if write_files:
                self._write_view(camera_number, fr)
                tm["write_wait"] += time.perf_counter() - t1
        if write_files:
            t0 = time.perf_counter()
            self._writer.flush()
            tm["write_wait"] += time.perf_counter() - t0
        tm["total"] = time.perf_counter() - t_run

    def close(self):
        """stop the writer thread (``run`` starts a new one when it needs it)"""
        if self._writer is not None:
            self._writer.close()
            self._writer = None

    def _write_view(self, camera_number, fr):
        view_dir = self.renderer.render_folder_name(camera_number)
        out_dir = os.path.join(view_dir, f"out_{self.model_name}")
        os.makedirs(out_dir, exist_ok=True)
        left = os.path.join(view_dir, "left.png")
        on_device = fr["depth"].is_cuda
        arrays = [(os.path.join(out_dir, "depth.npy"), fr["depth"]),
                  (os.path.join(out_dir, "occlusion_mask.npy"), fr["occlusion"].to(bool)), (left, fr["image"])]
        if not on_device:       # the writer downloads device tensors on its side stream; host tensors go as arrays
            arrays = [(p, a.numpy()) for p, a in arrays]
        ready = None
        if on_device:
            import torch
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(fr["depth"].device))

        def extra(host):
            from PIL import Image as PILImage
            PILImage.fromarray(np.ascontiguousarray(host[left]), mode="RGB").save(left)

        self._writer.submit(ready, arrays, extra)
