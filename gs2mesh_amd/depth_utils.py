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
  * the occlusion mask of the layout is ``alpha >= alpha_min``: a free foreground mask where no object masker exists.
No gradient flows through any of it.
"""
from __future__ import annotations

import os

import numpy as np

from .stereo_utils import _ViewWriter

KINDS = {"median": "median_depth", "expected": "depth"}


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
            out = render(cam, gaussians, getattr(self.args, "pipe", None), background, return_depth=True)
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
