"""The depth stage: drop-in for ``gs2mesh_utils.stereo_utils.Stereo`` with a pluggable matcher, the built-in HIP
semi-global matcher, and the disparity post-processing on the device.

``Stereo`` (below) walks the views like the reference's ``Stereo.run``; its matcher is either the built-in one
(``stereo_model="SGM"``, ``sgm_disparity`` / ``gs2m_stereo_sgm``) or a callable the caller supplies.  A stereo network
(DLNR, PyTorch) stays outside the package and plugs in through ``matcher=``.  What sits between the matcher and the TSDF
is small data-parallel work the reference does in numpy on the host with four ``np.save`` round trips per view:

  * ``get_occlusion_mask(L2R, R2L, threshold)``   stereo_utils.py:149-179 (left-right consistency)
  * ``depth = fx * baseline / disparity_LR``      stereo_utils.py:133

``depth_and_occlusion`` fuses both into one HIP kernel whose outputs (depth f32, mask u8) are exactly
the ``depth`` / ``mask`` inputs of ``ScalableTSDFVolume.integrate``.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from ._lib import _empty, _ptr, _stream_of


def depth_and_occlusion(disparity_LR, disparity_RL, fx, baseline, occlusion_threshold=3, want_depth=True,
                        want_mask=True, lib=None, stream=None):
    """-> (depth [H,W] f32 or None, visible_mask [H,W] u8 (1 = visible) or None), device tensors."""
    lib = lib or _lib.get()
    H, W = int(disparity_LR.shape[0]), int(disparity_LR.shape[1])
    depth = _empty(disparity_LR, (H, W), np.float32) if want_depth else None
    mask = _empty(disparity_LR, (H, W), np.uint8) if want_mask else None
    _lib.check(lib.gs2m_stereo_depth_occlusion(_ptr(disparity_LR), _ptr(disparity_RL) if want_mask else None, W, H,
                                               float(fx) * float(baseline), float(occlusion_threshold), _ptr(depth),
                                               _ptr(mask), _stream_of(disparity_LR, stream)), lib)
    return depth, mask


def get_occlusion_mask(L2R_disparity, R2L_disparity, occlusion_threshold, lib=None):
    """Same name / arguments / meaning as Stereo.get_occlusion_mask: boolean array, True = visible."""
    _, mask = depth_and_occlusion(L2R_disparity, R2L_disparity, 1.0, 1.0, occlusion_threshold, want_depth=False, lib=lib)
    return mask.astype(bool) if isinstance(mask, np.ndarray) else mask.to(bool)


# ---------------------------------------------------------------------------------------------------------------------
# the built-in matcher
# ---------------------------------------------------------------------------------------------------------------------
SGM_P1, SGM_P2 = 10, 120
SGM_MAX_DISPARITY = 1024


def sgm_disparity(left_rgb8, right_rgb8, max_disparity, p1=SGM_P1, p2=SGM_P2, want_rl=True, tap=False, lib=None, stream=None):
    """``gs2m_stereo_sgm``: four-path semi-global matching on a 9 x 7 census (include/gs2mesh_amd.h states the arithmetic).
    ``left_rgb8`` / ``right_rgb8``: [H,W,3] u8 on the device (one eye each of ``render_pair_device``'s rgb8);
    ``max_disparity``: a multiple of 64 up to 1024.  -> ``(disp_lr, disp_rl[, cost])``: [H,W] f32 disparities of the left
    and of the right image (``disp_rl`` is None without ``want_rl``) and, with ``tap``, the summed cost S [H,W,D] u16 of the
    left-based pass.  Device tensors, asynchronous on the stream (numpy arrays on the emulator back-end).  The scratch is
    kept per device and stream and only grows."""
    lib = lib or _lib.get()
    if tuple(left_rgb8.shape) != tuple(right_rgb8.shape) or left_rgb8.ndim != 3 or left_rgb8.shape[2] != 3:
        raise ValueError(f"sgm_disparity: two [H,W,3] images, got {tuple(left_rgb8.shape)} and {tuple(right_rgb8.shape)}")
    H, W, D = int(left_rgb8.shape[0]), int(left_rgb8.shape[1]), int(max_disparity)
    need = int(lib.gs2m_stereo_sgm_scratch_bytes(W, H, D))
    if need < 0:
        raise ValueError(f"sgm_disparity: max_disparity must be a multiple of 64 in [64, {SGM_MAX_DISPARITY}] "
                         f"(got {D}) and the image at most 65535 rows (got {W} x {H})")
    st = _stream_of(left_rgb8, stream)
    scratch = _lib.scratch("sgm", left_rgb8, need, st)
    disp_lr = _empty(left_rgb8, (H, W), np.float32)
    disp_rl = _empty(left_rgb8, (H, W), np.float32) if want_rl else None
    cost = None
    if tap:
        if hasattr(left_rgb8, "is_cuda"):
            import torch
            cost = torch.empty((H, W, D), dtype=torch.uint16, device=left_rgb8.device)
        else:
            cost = np.empty((H, W, D), np.uint16)
    _lib.check(lib.gs2m_stereo_sgm(_ptr(left_rgb8, name="left_rgb8"), _ptr(right_rgb8, name="right_rgb8"), W, H, D, int(p1),
                                   int(p2), _ptr(disp_lr), _ptr(disp_rl), _ptr(scratch), scratch.shape[0] * 8, _ptr(cost), st), lib)
    return (disp_lr, disp_rl, cost) if tap else (disp_lr, disp_rl)


# ---------------------------------------------------------------------------------------------------------------------
# Stereo: drop-in for gs2mesh_utils.stereo_utils.Stereo
# ---------------------------------------------------------------------------------------------------------------------
class _ViewWriter:
    """Downloads and saves the arrays of finished views on a thread of its own, so the next view's kernels do not wait
    for the disk.  At most ``max_pending`` views are held; ``submit`` blocks beyond that.  ``flush`` returns when every
    submitted file is complete and re-raises the first error."""

    def __init__(self, max_pending=4):
        import queue
        import threading
        self._slots = threading.BoundedSemaphore(int(max_pending))
        self._jobs = queue.Queue()
        self._error = None
        self._copy = None       # side stream of the downloads
        self._thread = threading.Thread(target=self._run, name="gs2m-stereo-writer", daemon=True)
        self._thread.start()

    def submit(self, ready, arrays, extra=None):
        """``arrays``: list of (path, device tensor or host array) for np.save; ``ready``: torch event after which the
        tensors are complete (None for host arrays); ``extra``: callable(host arrays by path) run after the saves."""
        if self._error is not None:
            raise RuntimeError(f"Stereo writer: an earlier write failed: {self._error!r}") from self._error
        self._slots.acquire()
        self._jobs.put((ready, arrays, extra))

    def _download(self, ready, arrays):
        tensors = [a for _, a in arrays if hasattr(a, "is_cuda")]
        if not tensors:
            return {p: np.asarray(a) for p, a in arrays}
        import torch
        dev = tensors[0].device
        if self._copy is None:
            self._copy = torch.cuda.Stream(device=dev)
        host = {}
        with torch.cuda.device(dev), torch.cuda.stream(self._copy):
            if ready is not None:
                self._copy.wait_event(ready)
            for p, a in arrays:
                if hasattr(a, "is_cuda"):
                    h = torch.empty(a.shape, dtype=a.dtype, pin_memory=True)
                    h.copy_(a, non_blocking=True)
                    host[p] = h
                else:
                    host[p] = np.asarray(a)
        self._copy.synchronize()
        return {p: (h.numpy() if hasattr(h, "numpy") else h) for p, h in host.items()}

    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            try:
                ready, arrays, extra = job
                host = self._download(ready, arrays)
                if self._error is None:
                    for path, a in host.items():
                        if path.endswith(".npy"):
                            np.save(path, a)
                    if extra is not None:
                        extra(host)
            except BaseException as e:       # reported by flush() / the next submit()
                if self._error is None:
                    self._error = e
            finally:
                self._slots.release()
                self._jobs.task_done()

    def flush(self):
        self._jobs.join()
        if self._error is not None:
            raise self._error

    def close(self):
        if self._thread.is_alive():
            self._jobs.put(None)
            self._thread.join()


class Stereo:
    """Drop-in for ``gs2mesh_utils.stereo_utils.Stereo`` (stereo_utils.py:25-179): the reference's constructor plus
    ``matcher`` and ``lib``, ``model_name``, ``run(start, visualize)``, ``get_occlusion_mask`` and the on-disk layout
    ``<view>/out_<model>/{disparity_LR,disparity_RL,occlusion_mask,depth}.npy`` that ``TSDF``, ``Masker`` and a
    ``--skip_rendering`` resume read.

    The matcher is pluggable:
      * ``args.stereo_model == "SGM"``: the built-in HIP semi-global matcher (``sgm_disparity``).  It needs no weights and
        makes the path render -> depth -> fuse complete with this package alone; it is NOT the reference's DLNR network and
        does not claim its quality.  D = ``args.stereo_max_disparity`` if present, else the disparity of the nearest depth
        ``TSDF.run`` keeps (fx / TSDF_min_depth_baselines) rounded up to a multiple of 64; ``args.stereo_sgm_p1`` / ``_p2``
        are optional.  ``args.stereo_warm`` does not apply to it.
      * any other name: ``matcher(image1, image2) -> disparity``, a callable on two [1,3,H,W] float tensors (what the
        reference's ``load_image`` returns) giving the positive disparity of image1's pixels as [H,W] (leading singleton
        dimensions are squeezed).  It is called as the reference calls its network: ``(left, right)`` for LR and
        ``(flip(right), flip(left))``, flipped back, for RL.  Padding, the network's sign and a warm start live in it.

    Per view ``run`` does one ``renderer.render_pair_device`` (no PNG read-back), the two matcher passes and
    ``depth_and_occlusion``; everything stays on the device and the files are written behind it by a writer thread (all
    complete when ``run`` returns).  Deviation from the reference: its five visualisation images are written only with
    ``save_visuals=True`` (matplotlib / PIL).  ``keep_on_device=True`` keeps ``left`` / ``depth`` / ``occlusion`` of every view
    and ``frame_source`` hands them to ``TSDF(..., frame_source=stereo.frame_source)``; ``write_files=False`` skips the disk."""

    def __init__(self, base_dir, renderer, args, device='cuda', matcher=None, lib=None):
        self.base_dir = base_dir
        self.renderer = renderer
        self.args = args
        self.model_name = args.stereo_model
        self.device = device
        self.matcher = matcher
        self._lib = lib                  # None = the HIP library (tests inject the emulator build)
        self.frames = {}                 # keep_on_device: camera number -> dict(image, depth, occlusion)
        self.timings = {}                # host wall seconds of the last run(): render, match, post, write_wait, total
        self._writer = None
        if self.model_name == "SGM":
            if matcher is not None:
                raise ValueError('stereo_model "SGM" is the built-in matcher: pass either that name or a matcher')
            self.sgm_p1 = int(getattr(args, "stereo_sgm_p1", SGM_P1))
            self.sgm_p2 = int(getattr(args, "stereo_sgm_p2", SGM_P2))
            if getattr(args, "stereo_warm", False):
                print('Stereo: stereo_warm does not apply to the "SGM" matcher (ignored)')
        elif matcher is None:
            raise RuntimeError(f'stereo_model {self.model_name!r} is not built in (only "SGM" is): pass '
                               "matcher=callable(image1, image2) -> disparity, e.g. a wrapped DLNR network")

    # -- matchers -----------------------------------------------------------------------------------------------------
    def max_disparity(self, camera):
        """D of the built-in matcher for a view"""
        D = getattr(self.args, "stereo_max_disparity", None)
        if D is None:
            D = 64 * int(np.ceil(camera['fx'] / self.args.TSDF_min_depth_baselines / 64.0))
        D = int(D)
        if D > SGM_MAX_DISPARITY:
            raise ValueError(f"Stereo: the SGM matcher searches at most {SGM_MAX_DISPARITY} disparities, this view needs {D} "
                             "(set args.stereo_max_disparity, raise TSDF_min_depth_baselines or render smaller)")
        return D

    def _match(self, rgb8, camera):
        """-> (disparity_LR, disparity_RL), [H,W] f32 where rgb8 lives"""
        if self.model_name == "SGM":
            return sgm_disparity(rgb8[0], rgb8[1], self.max_disparity(camera), self.sgm_p1, self.sgm_p2,
                                 lib=self._lib)
        import torch
        on_host = isinstance(rgb8, np.ndarray)
        t = torch.from_numpy(rgb8) if on_host else rgb8
        image1 = t[0].permute(2, 0, 1).float()[None]
        image2 = t[1].permute(2, 0, 1).float()[None]
        H, W = int(t.shape[1]), int(t.shape[2])

        def disparity(d):
            d = torch.as_tensor(d).detach()
            return d.reshape(H, W).to(torch.float32)

        with torch.no_grad():
            lr = disparity(self.matcher(image1, image2))
            rl = torch.flip(disparity(self.matcher(torch.flip(image2, dims=[3]), torch.flip(image1, dims=[3]))), dims=[1])
        if on_host:
            return np.ascontiguousarray(lr.cpu().numpy()), np.ascontiguousarray(rl.cpu().numpy())
        return lr.to(t.device).contiguous(), rl.to(t.device).contiguous()

    def get_occlusion_mask(self, L2R_disparity, R2L_disparity, occlusion_threshold):
        return get_occlusion_mask(L2R_disparity, R2L_disparity, occlusion_threshold, lib=self._lib)

    def frame_source(self, camera_number):
        """for ``TSDF(..., frame_source=stereo.frame_source)`` after ``run(keep_on_device=True)``"""
        try:
            return self.frames[camera_number]
        except KeyError:
            raise RuntimeError(f"Stereo.frame_source: view {camera_number} was not kept "
                               "(run(keep_on_device=True) from a start that covers it)") from None

    # -- run ----------------------------------------------------------------------------------------------------------
    def run(self, start=0, visualize=False, keep_on_device=False, write_files=True, save_visuals=False):
        import time
        tm = self.timings = dict(render=0.0, match=0.0, post=0.0, write_wait=0.0, total=0.0)
        t_run = time.perf_counter()
        ren, a = self.renderer, self.args
        if write_files and self._writer is None:
            self._writer = _ViewWriter()
        device_png = getattr(ren, "png_encoder", "pil") == "device"
        for camera_number, left_camera in enumerate(ren.left_cameras):
            if camera_number < start:
                continue
            t0 = time.perf_counter()
            rgb8 = ren.render_pair_device(camera_number)["rgb8"]
            t1 = time.perf_counter()
            disp_lr, disp_rl = self._match(rgb8, left_camera)
            t2 = time.perf_counter()
            depth, occ = depth_and_occlusion(disp_lr, disp_rl, left_camera['fx'], ren.baseline,
                                             a.stereo_occlusion_threshold, lib=self._lib)
            t3 = time.perf_counter()
            tm["render"] += t1 - t0
            tm["match"] += t2 - t1
            tm["post"] += t3 - t2
            if keep_on_device:
                self.frames[camera_number] = dict(image=rgb8[0], depth=depth, occlusion=occ)
            if write_files:
                self._write_view(camera_number, rgb8, disp_lr, disp_rl, depth, occ, device_png, save_visuals)
                tm["write_wait"] += time.perf_counter() - t3
            if visualize:
                d = _lib.MEMORY.download(depth)
                print(f"baseline: {ren.baseline}")
                print(f"minimal depth: {d.min()}, maximal depth: {d.max()}")
        if write_files:
            t0 = time.perf_counter()
            self._writer.flush()
            if hasattr(ren, "flush"):
                ren.flush()
            tm["write_wait"] += time.perf_counter() - t0
        tm["total"] = time.perf_counter() - t_run

    def close(self):
        """stop the writer thread (``run`` starts a new one when it needs it)"""
        if self._writer is not None:
            self._writer.close()
            self._writer = None

    def _write_view(self, camera_number, rgb8, disp_lr, disp_rl, depth, occ, device_png, save_visuals):
        ren = self.renderer
        out_dir = os.path.join(ren.render_folder_name(camera_number), f'out_{self.model_name}')
        os.makedirs(out_dir, exist_ok=True)
        on_device = hasattr(depth, "is_cuda") and depth.is_cuda
        occ_bool = occ.to(bool) if hasattr(occ, "is_cuda") else np.asarray(occ).astype(bool)
        arrays = [(os.path.join(out_dir, "disparity_LR.npy"), disp_lr), (os.path.join(out_dir, "disparity_RL.npy"), disp_rl),
                  (os.path.join(out_dir, "occlusion_mask.npy"), occ_bool), (os.path.join(out_dir, "depth.npy"), depth)]
        if device_png:                       # encoded on the device, on this thread's stream; written by the renderer's writer
            ren.write_pair(camera_number, rgb8, wait=False)
        else:
            arrays.append(("rgb8", rgb8))
        ready = None
        if on_device:
            import torch
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(depth.device))

        def extra(host):
            if not device_png:
                ren.write_pair(camera_number, host["rgb8"])
            if save_visuals:
                _save_visuals(out_dir, {os.path.basename(p): v for p, v in host.items()},
                              getattr(self.args, "stereo_shading_eps", 1e-4))

        self._writer.submit(ready, arrays, extra)


def _save_visuals(out_dir, host, shading_eps):
    """the reference's visualisation files (stereo_utils.py:130-140) without cv2: jet-mapped disparities, the mask, the depth
    saturated to 8 bits and a Sobel shading image"""
    import matplotlib
    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from PIL import Image as PILImage
    from scipy import ndimage
    for d in ("LR", "RL"):
        plt.imsave(os.path.join(out_dir, f"disparity_{d}.png"), host[f"disparity_{d}.npy"], cmap='jet')
    plt.imsave(os.path.join(out_dir, "occlusion_mask.png"), host["occlusion_mask.npy"])
    depth = np.nan_to_num(host["depth.npy"], posinf=0.0)
    PILImage.fromarray(np.clip(np.rint(depth), 0, 255).astype(np.uint8)).save(os.path.join(out_dir, "depth.png"))
    gx, gy = ndimage.sobel(depth, axis=1), ndimage.sobel(depth, axis=0)
    shading = 1.0 / np.sqrt(gx * gx + gy * gy + float(shading_eps))
    shading = shading / max(float(shading.max()), 1e-30)
    PILImage.fromarray(np.clip(np.rint(shading * 255.0), 0, 255).astype(np.uint8)).save(os.path.join(out_dir, "shading.png"))
