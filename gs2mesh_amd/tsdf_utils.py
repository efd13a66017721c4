"""Pipeline-level drop-in for ``gs2mesh_utils.tsdf_utils.TSDF`` (tsdf_utils.py:23-142), fuse half.

``TSDF(renderer, stereo, args, out_name).run()`` walks the views exactly like the reference
(TSDF_dilate / TSDF_valid / TSDF_skip, masks, occlusion mask, min / max depth in baselines,
TSDF_scale on the extrinsic translation and the depth) and integrates them with the HIP block-sparse
volume instead of Open3D's CPU ``ScalableTSDFVolume``.  The per-pixel preprocessing
(depth *= mask, depth < min -> 0, depth/scale, >= trunc -> 0; tsdf_utils.py:68-93) is fused into the
integration kernels; only the 10x10 closing + erosion of the object mask (tsdf_utils.py:73-77) stays on
the host (scipy.ndimage; cv2 is not a dependency).  Frames can come from disk (``left.png``,
``out_<model>/depth.npy``, ...: the reference layout, so ``--skip_rendering`` style resumes work) or
from memory via ``frame_source`` (the in-memory hand-off).

``TSDF(..., consistency=...)`` (or ``args.TSDF_consistency``) puts the cross-view test of ``depth_utils.depth_consistency`` in
front of the fusion: the depth maps of all selected cameras vote on each other once, and each frame is then fused under its
keep mask.  Off by default, and the reference has no such stage.

``TSDF(..., fuse="batch")`` (or ``args.TSDF_fuse = "batch"``) fuses the same frames into the same volume (every block, every
voxel bit for bit) in sweeps of at most ``MAX_SWEEP`` frames: a thread pool reads the next sweep from disk while the current one is integrated,
the masks of a sweep are preprocessed on the device in one call (``mask_preprocess``, ``gs2m_mask_preprocess``), the sweep
is one ``integrate_batch`` and the vertex normals are computed on the device.  The mesh is the same mesh; its vertex and
triangle ORDER follows the volume's block slots, which atomics hand out in either path (two runs of one path differ in it
too), so meshes compare by their cut-edge keys (``mesh.edge_index``), and the vertex normals, summed in triangle order, agree
to rounding (each equals the host statement on its own mesh bit for bit).  The default, ``fuse="frame"``, is the loop above.

After ``run()``: ``self.volume`` (gs2mesh_amd.integration.ScalableTSDFVolume) and ``self.mesh`` (marching
cubes on the GPU, ``gs2m_tsdf_extract``); ``save_mesh`` / ``clean_mesh`` write the reference's
``<out_name>_mesh.ply`` / ``<out_name>_cleaned_mesh.ply`` (tsdf_utils.py:112-142).
"""
from __future__ import annotations

import ctypes as C
import os
import time
from concurrent.futures import Future, ThreadPoolExecutor

import numpy as np

from . import _lib
from .integration import (Image, PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume,
                          TSDFVolumeColorType)


def _morph(m, k, erode):
    """cv2.erode / cv2.dilate with a k x k box of ones, default anchor (k//2, k//2) and default constant
    border (+inf for erode, -inf for dilate):  dst(y,x) = min|max over dy,dx in [-k//2, k-1-k//2] of
    src(y+dy, x+dx).  Written with explicit offsets so that even kernel sizes (10, the reference
    default) are unambiguous."""
    a = k // 2
    b = k - 1 - a
    pad = np.pad(m, ((a, b), (a, b)), constant_values=bool(erode))
    # separable: a box is the product of a row and a column segment
    win = np.lib.stride_tricks.sliding_window_view(pad, k, axis=1)
    r = win.all(axis=-1) if erode else win.any(axis=-1)
    win = np.lib.stride_tricks.sliding_window_view(r, k, axis=0)
    return win.all(axis=-1) if erode else win.any(axis=-1)


def preprocess_object_mask(mask, invert=False, erode=True, closing_kernel_size=10, erosion_kernel_size=10):
    """tsdf_utils.py:69-77: optional inversion, then cv2.MORPH_CLOSE (dilate, erode) and cv2.erode with
    k x k boxes of ones; returns a bool mask."""
    m = np.asarray(mask).astype(bool)
    if invert:
        m = ~m
    if erode:
        m = _morph(_morph(m, closing_kernel_size, erode=False), closing_kernel_size, erode=True)
        m = _morph(m, erosion_kernel_size, erode=True)
    return m


def _u8_mask(m):
    """a mask (host array or tensor of any dtype, non-zero = true) as the u8 the kernel reads (non-zero = true): bool and
    uint8 masks as they are"""
    if hasattr(m, "is_cuda"):                     # torch tensor
        import torch
        return m if m.dtype in (torch.uint8, torch.bool) else m != 0
    m = np.asarray(m)
    if m.dtype == np.bool_:
        return m.view(np.uint8)
    return m if m.dtype == np.uint8 else (m != 0).view(np.uint8)


def mask_preprocess(object_masks, occlusion_masks=None, invert=False, erode=True, closing_kernel_size=10,
                    erosion_kernel_size=10, lib=None, device=0):
    """``gs2m_mask_preprocess``: for every frame, ``preprocess_object_mask(object_mask, invert, erode, closing, erosion) &
    occlusion_mask`` as a device u8 mask (0 / 1), all frames in one call.  ``object_masks`` / ``occlusion_masks``: lists of
    [H,W] host arrays or device tensors (non-zero = true), or None; an entry (or a whole list) of None is an absent mask.
    Returns the list of device masks (views of one [n,H,W] buffer), None where a frame has neither mask.  Runs on torch's
    current stream: the uploads and the scratch this call drops are released in that stream's order."""
    if object_masks is None and occlusion_masks is None:
        raise ValueError("mask_preprocess: no masks")
    n = len(object_masks) if object_masks is not None else len(occlusion_masks)
    objs = list(object_masks) if object_masks is not None else [None] * n
    occs = list(occlusion_masks) if occlusion_masks is not None else [None] * n
    if len(objs) != n or len(occs) != n:
        raise ValueError("mask_preprocess: object_masks and occlusion_masks must have the same length")
    k1, k2 = int(closing_kernel_size), int(erosion_kernel_size)
    if erode and (k1 < 1 or k2 < 1):
        raise ValueError(f"mask_preprocess: kernel sizes must be >= 1 (closing {k1}, erosion {k2})")
    shapes = {tuple(m.shape) for m in objs + occs if m is not None}
    if not shapes:
        return [None] * n
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError(f"mask_preprocess: the masks must share one [H,W] shape, got {sorted(shapes)}")
    H, W = next(iter(shapes))
    import torch
    lib = lib if lib is not None else _lib.get()
    mem = _lib.MEMORY
    obj_p, occ_p, out_p = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    with_mask = [objs[i] is not None or occs[i] is not None for i in range(n)]
    # the kernel writes every pixel of every output: no fill
    out_all = mem.empty((sum(with_mask), H, W), np.uint8, device)
    keep, outs = [], []
    for i in range(n):
        o = mem.upload(_u8_mask(objs[i]), torch.uint8, device) if objs[i] is not None else None
        c = mem.upload(_u8_mask(occs[i]), torch.uint8, device) if occs[i] is not None else None
        out = out_all[len([x for x in outs if x is not None])] if with_mask[i] else None
        keep += [o, c]
        outs.append(out)
        obj_p[i], occ_p[i], out_p[i] = mem.ptr(o), mem.ptr(c), mem.ptr(out)
    morph = bool(erode) and any(o is not None for o in objs)
    # every scratch word is written before it is read
    scratch = mem.empty((2 * n * H * ((W + 63) // 64),), np.int64, device) if morph else None
    st = mem.current_stream(device)
    _lib.check(lib.gs2m_mask_preprocess(n, W, H, obj_p, occ_p, int(bool(invert)), int(bool(erode)), max(k1, 1), max(k2, 1), out_p,
                                        mem.ptr(scratch), st), lib)
    return outs


class TSDF:
    MAX_SWEEP = 32          # frames per integrate_batch sweep of fuse="batch" (equal sweeps of at most this many)
    LOADER_THREADS = 8      # disk readers of fuse="batch" (capped by the CPUs this process may use)
    CONSISTENCY_MAX_BYTES = 8 << 30     # consistency: all selected depth maps (and their masks) are resident at once, up to this

    def __init__(self, renderer, stereo, args, out_name, frame_source=None, max_blocks=None, lib=None, fuse=None,
                 consistency=None):
        self.model_name = stereo.model_name if stereo is not None else getattr(args, "stereo_model", "DLNR_Middlebury")
        self.renderer = renderer
        self.out_name = out_name
        self.args = args
        self.frame_source = frame_source      # callable(camera_number) -> dict(image, depth[, mask, occlusion])
        self.max_blocks = max_blocks
        self._lib = lib                       # None = the HIP library (tests inject the emulator build)
        self.volume = None
        self.mesh = None
        self.fuse = fuse if fuse is not None else getattr(args, "TSDF_fuse", "frame")
        if self.fuse not in ("frame", "batch"):
            raise ValueError(f"fuse must be 'frame' or 'batch', got {self.fuse!r}")
        self.timings = {}       # wall seconds per stage of the last run(): fuse, extract, normals (+ load_wait, mask, integrate: batch;
                                # + consistency, a part of fuse, when the filter is on)
        # the cross-view filter: a ConsistencyParams, a dict of its fields or True (the defaults); None = off.  Without the
        # argument, args.TSDF_consistency (same forms) and args.TSDF_consistency_<field> say it; an args without them: off
        self.consistency = self._consistency_params(consistency, args)
        self._keep_masks = None     # during run(): camera number -> device keep mask
        if self.consistency is not None:
            self._consistency_bytes(self._selected())         # over the cap: refuse here, before anything is loaded

    def _load_frame(self, camera_number):
        if self.frame_source is not None:
            return self.frame_source(camera_number)
        from PIL import Image as PILImage
        a = self.args
        d = self.renderer.render_folder_name(camera_number)
        fr = dict(image=np.array(PILImage.open(os.path.join(d, 'left.png'))).astype(np.uint8),
                  depth=np.load(os.path.join(d, f'out_{self.model_name}', 'depth.npy')))
        if a.TSDF_use_mask:
            fr["mask"] = np.load(os.path.join(d, 'left_mask.npy')).astype(bool)
        if a.TSDF_use_occlusion_mask:
            fr["occlusion"] = np.load(os.path.join(d, f'out_{self.model_name}', 'occlusion_mask.npy')).astype(bool)
        return fr

    def _selected(self):
        """camera numbers to fuse, in order (TSDF_dilate / TSDF_valid / TSDF_skip; tsdf_utils.py:60-66)"""
        a = self.args
        n = len(self.renderer)
        valid = a.TSDF_valid if a.TSDF_valid is not None else list(range(n))
        skip = a.TSDF_skip if a.TSDF_skip is not None else []
        out = []
        for camera_number, _ in enumerate(self.renderer.left_cameras):
            if camera_number % a.TSDF_dilate != 0:
                continue
            if valid is not None and camera_number not in valid:
                continue
            if skip is not None and camera_number in skip:
                continue
            out.append(camera_number)
        return out

    def _intrinsic(self, camera_number):
        c = self.renderer.left_cameras[camera_number]
        return PinholeCameraIntrinsic(c['width'], c['height'], c['fx'], c['fy'], c['cx'], c['cy'])

    def _world_to_camera(self, camera_number):
        extrinsic = self.renderer.left_cameras[camera_number]['extrinsic'].copy()
        extrinsic[:3, 3] /= self.args.TSDF_scale
        return np.linalg.inv(extrinsic)

    @staticmethod
    def _consistency_params(consistency, args):
        import dataclasses
        from .depth_utils import ConsistencyParams
        if consistency is not None:
            return ConsistencyParams.coerce(consistency)
        p = ConsistencyParams.coerce(getattr(args, "TSDF_consistency", None))
        if p is None:
            return None
        over = {f.name: getattr(args, "TSDF_consistency_" + f.name) for f in dataclasses.fields(ConsistencyParams)
                if getattr(args, "TSDF_consistency_" + f.name, None) is not None}
        return dataclasses.replace(p, **over) if over else p

    def _consistency_bytes(self, cameras):
        """bytes the filter keeps on the device for ``cameras``: depth f32 + keep u8 (+ occlusion u8) per pixel"""
        per_pixel = 4 + 1 + (1 if self.args.TSDF_use_occlusion_mask else 0)
        need = sum(per_pixel * int(self.renderer.left_cameras[c]['width']) * int(self.renderer.left_cameras[c]['height'])
                   for c in cameras)
        if need > int(self.CONSISTENCY_MAX_BYTES):
            raise RuntimeError(f"TSDF consistency: the {len(cameras)} selected depth maps need {need} bytes on the device at once, "
                               f"above TSDF.CONSISTENCY_MAX_BYTES = {int(self.CONSISTENCY_MAX_BYTES)}; fuse fewer views (TSDF_dilate / "
                               "TSDF_valid / TSDF_skip), raise the cap or run without consistency (there is no windowed mode)")
        return need

    def _consistency_keep(self, volume):
        """camera number -> device u8 keep mask (``depth_utils.depth_consistency``) over the depth maps of ``_selected()``, one
        call.  A pixel has a depth where ``run`` would fuse it: inside the min / max depth range (unscaled units) and, with
        TSDF_use_occlusion_mask, on the frame's occlusion mask -- so a keep mask lies inside the occlusion mask and stands in
        for it when the frame is fused.  Disk frames are read here for their depth and occlusion mask and again by the fusion."""
        from .depth_utils import depth_consistency
        t0 = time.perf_counter()
        a = self.args
        cams = self._selected()
        self._consistency_bytes(cams)
        depths, occs, intr = [], [], []
        for c in cams:
            fr = self._load_frame(c)
            i = self._intrinsic(c)
            if tuple(fr["depth"].shape) != (i.height, i.width):
                raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
            depths.append(fr["depth"])
            occs.append(fr.get("occlusion") if a.TSDF_use_occlusion_mask else None)
            intr.append(i)
        poses = np.stack([np.asarray(self.renderer.left_cameras[c]['extrinsic'], np.float64) for c in cams]) if cams else \
            np.zeros((0, 4, 4))
        baseline = self.renderer.baseline
        keep = depth_consistency(depths, intr, poses, self.consistency, masks=occs if any(o is not None for o in occs) else None,
                                 min_depth=a.TSDF_min_depth_baselines * baseline, max_depth=a.TSDF_max_depth_baselines * baseline,
                                 lib=volume._lib, device=volume.device)
        # host wall time of getting the frames and queueing the one call; the kernels' own time is not in it (nothing waits
        # for them here): it shows in whatever synchronises next, and tools/consistency_bench.py measures it with events
        self._consistency_time = time.perf_counter() - t0
        return dict(zip(cams, keep))

    def _sweeps(self, cameras):
        """consecutive cameras sharing one intrinsic, cut into equal sweeps of at most MAX_SWEEP (bench.py's rule)"""
        groups = []
        for c in cameras:
            i = self._intrinsic(c)
            key = (i.width, i.height, i.fx, i.fy, i.cx, i.cy)
            if groups and groups[-1][0] == key:
                groups[-1][1].append(c)
            else:
                groups.append((key, [c]))
        sweeps = []
        for _, g in groups:
            size = -(-len(g) // -(-len(g) // int(self.MAX_SWEEP)))
            sweeps += [g[i:i + size] for i in range(0, len(g), size)]
        return sweeps

    def run(self, visualize=False):
        a = self.args
        self._t_start = time.perf_counter()
        voxel_length = a.TSDF_voxel / 512
        kw = {} if self.max_blocks is None else dict(max_blocks=self.max_blocks)
        if self._lib is not None:
            kw["lib"] = self._lib
        volume = ScalableTSDFVolume(voxel_length=float(voxel_length), sdf_trunc=a.TSDF_sdf_trunc,
                                    color_type=TSDFVolumeColorType.RGB8, **kw)
        if self.consistency is not None:
            try:
                self._keep_masks = self._consistency_keep(volume)
                return self._fuse(volume)
            finally:                                    # also when a frame fails to load: the device masks do not outlive run()
                self._keep_masks = None
        return self._fuse(volume)

    def _fuse(self, volume):
        a = self.args
        baseline = self.renderer.baseline
        if self.fuse == "batch":
            self._fuse_batch(volume)
            return self._finish(volume, on_device=True)
        for camera_number in self._selected():
            fr = self._load_frame(camera_number)
            if self._keep_masks is not None:                  # the keep mask lies inside the occlusion mask: it takes its place
                fr = dict(fr, occlusion=_lib.MEMORY.download(self._keep_masks[camera_number]))
            mask = None
            if a.TSDF_use_mask and fr.get("mask") is not None:
                mask = preprocess_object_mask(fr["mask"], a.TSDF_invert_mask, a.TSDF_erode_mask,
                                              a.TSDF_closing_kernel_size, a.TSDF_erosion_kernel_size)
            if (a.TSDF_use_occlusion_mask or self._keep_masks is not None) and fr.get("occlusion") is not None:
                occ = fr["occlusion"]
                occ = np.asarray(occ.cpu() if hasattr(occ, "cpu") else occ).astype(bool)
                mask = occ if mask is None else (np.asarray(mask).astype(bool) & occ)
            if mask is not None:
                mask = np.asarray(mask).astype(np.uint8)
            depth_trunc = baseline * a.TSDF_max_depth_baselines / a.TSDF_scale
            rgbd = RGBDImage.create_from_color_and_depth(Image(fr["image"]), Image(fr["depth"]),
                                                         depth_scale=a.TSDF_scale, depth_trunc=depth_trunc,
                                                         convert_rgb_to_intensity=False)
            volume.integrate(rgbd, self._intrinsic(camera_number), self._world_to_camera(camera_number), mask=mask,
                             min_depth=a.TSDF_min_depth_baselines * baseline)
        self._finish(volume, on_device=False)

    def _finish(self, volume, on_device):
        a = self.args
        volume.status()
        t0 = time.perf_counter()
        self.timings["fuse"] = t0 - self._t_start           # selection, loading and integration, up to the last voxel written
        self.volume = volume
        self.mesh = volume.extract_triangle_mesh()                  # tsdf_utils.py:108
        self.mesh.scale(a.TSDF_scale, (0, 0, 0))                    # :109
        t1 = time.perf_counter()
        if on_device:
            self.mesh.compute_vertex_normals(on_device=True, lib=volume._lib, device=volume.device)
        else:
            self.mesh.compute_vertex_normals()                      # :110
        t2 = time.perf_counter()
        self.timings.update(extract=t1 - t0, normals=t2 - t1)
        if self._keep_masks is not None:
            self.timings["consistency"] = self._consistency_time

    def _fuse_batch(self, volume):
        """fuse="batch": the frames of ``_selected()`` in order, sweep by sweep.  Disk frames are read by a thread pool one sweep
        ahead (at most two sweeps of frames are held); ``frame_source`` frames are fetched on this thread."""
        sweeps = self._sweeps(self._selected())
        tm = self.timings = dict(load_wait=0.0, mask=0.0, integrate=0.0)
        pool = None
        if self.frame_source is None and sweeps:
            workers = max(1, min(int(self.LOADER_THREADS), len(os.sched_getaffinity(0))))
            pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="tsdf-load")

        def submit(cams):
            if pool is None:
                return [self._load_frame(c) for c in cams]
            return [pool.submit(self._load_frame, c) for c in cams]

        try:
            pending = submit(sweeps[0]) if sweeps else []
            for i, cams in enumerate(sweeps):
                t0 = time.perf_counter()
                frames = [f.result() if isinstance(f, Future) else f for f in pending]
                pending = submit(sweeps[i + 1]) if i + 1 < len(sweeps) else []
                tm["load_wait"] += time.perf_counter() - t0
                self._integrate_sweep(volume, cams, frames)
                del frames
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)

    def _integrate_sweep(self, volume, cams, frames):
        """one gs2m_mask_preprocess + one integrate_batch for the frames of one sweep (one intrinsic)"""
        a = self.args
        baseline = self.renderer.baseline
        depth_trunc = baseline * a.TSDF_max_depth_baselines / a.TSDF_scale
        intr = self._intrinsic(cams[0])
        images, objs, occs = [], [], []
        for fr in frames:
            images.append(RGBDImage.create_from_color_and_depth(Image(fr["image"]), Image(fr["depth"]),
                                                                depth_scale=a.TSDF_scale, depth_trunc=depth_trunc,
                                                                convert_rgb_to_intensity=False))
            objs.append(fr.get("mask") if a.TSDF_use_mask else None)
            occs.append(fr.get("occlusion") if a.TSDF_use_occlusion_mask else None)
        if self._keep_masks is not None:                      # a keep mask lies inside its frame's occlusion mask: it takes its place
            occs = [self._keep_masks[c] for c in cams]
        t0 = time.perf_counter()
        masks = None
        if any(m is not None for m in objs + occs):
            if any(tuple(m.shape) != (intr.height, intr.width) for m in objs + occs if m is not None):
                raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
            masks = mask_preprocess(objs, occs, a.TSDF_invert_mask, a.TSDF_erode_mask, a.TSDF_closing_kernel_size,
                                    a.TSDF_erosion_kernel_size, lib=volume._lib, device=volume.device)
        t1 = time.perf_counter()
        volume.integrate_batch(images, intr, [self._world_to_camera(c) for c in cams], masks=masks,
                               min_depth=a.TSDF_min_depth_baselines * baseline)
        self.timings["mask"] += t1 - t0
        self.timings["integrate"] += time.perf_counter() - t1

    def save_mesh(self):
        """tsdf_utils.py:112-120."""
        from .mesh import write_triangle_mesh
        write_triangle_mesh(os.path.join(self.renderer.output_dir_root, f'{self.out_name}_mesh.ply'), self.mesh)
        print("SAVED MESH")

    def clean_mesh(self):
        """tsdf_utils.py:122-142: drop connected components with fewer than TSDF_cleaning_threshold / TSDF_scale
        triangles.  As in the reference the method rebinds ``self.clean_mesh`` to the cleaned mesh (:138)."""
        import copy
        from .mesh import write_triangle_mesh
        thres = self.args.TSDF_cleaning_threshold / self.args.TSDF_scale
        triangle_clusters, cluster_n_triangles, cluster_area = self.mesh.cluster_connected_triangles()
        triangles_to_remove = cluster_n_triangles[triangle_clusters] < thres
        self.clean_mesh = copy.deepcopy(self.mesh)
        self.clean_mesh.remove_triangles_by_mask(triangles_to_remove)
        self.clean_mesh.remove_unreferenced_vertices()
        write_triangle_mesh(os.path.join(self.renderer.output_dir_root, f'{self.out_name}_cleaned_mesh.ply'),
                            self.clean_mesh)
        print("SAVED CLEANED MESH")
