"""Operator-level drop-in for the reference's ``diff_gaussian_rasterization`` module
(DGR/diff_gaussian_rasterization/__init__.py): forward pass and, for 3DGS training, the backward pass.

Same public names, argument meaning and error behaviour:

    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rasterizer = GaussianRasterizer(raster_settings=GaussianRasterizationSettings(...))
    color, radii = rasterizer(means3D=..., means2D=..., shs=..., colors_precomp=None, opacities=...,
                              scales=..., rotations=..., cov3D_precomp=None)

``GS/gaussian_renderer/__init__.py:14`` imports exactly these two names, so putting this package on
``sys.path`` as ``diff_gaussian_rasterization`` makes the reference's ``render()`` run
on the HIP kernels unchanged.  The hot path runs under ``torch.no_grad()``
(gs2mesh_utils/renderer_utils.py:374) and takes the plain forward.  When gradients are enabled and an input requires grad, the
call goes through ``_RasterizeGaussians`` (the reference's autograd Function, DGR __init__.py:44-155: same signature, same
gradient tuple): ``loss.backward()`` fills ``.grad`` of means3D, means2D (NDC-scaled, what densification reads), shs /
colors_precomp, opacities, scales, rotations and cov3D_precomp with the reference's gradients (``gs2m_rasterize_backward``).
The forward state the backward needs stays in the per-device handle; if another forward ran on the handle in between, the
backward first replays its own forward into a scratch image, so correctness never depends on call order.
All tensors must be float32, contiguous and on the HIP device; outputs are freshly allocated.

Extension (the reference renders colour only): ``GaussianRasterizer.forward(..., return_depth=True)`` returns
``(color, radii, expected, median, alpha)`` -- the depth and opacity maps of ``gs2m_rasterize_depth`` -- and, when gradients are
wanted, goes through ``_RasterizeGaussiansDepth``, whose backward hands the upstream gradients of the image and of the three
maps to ONE ``gs2m_rasterize_backward_depth`` call: a depth-supervised or depth-regularised loss trains the splat.  The keyword
defaults to False and the reference's 2-tuple is untouched.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from ..rasterizer import Rasterizer

_HANDLES = {}


def _handle(device: torch.device) -> Rasterizer:
    """One persistent arena set per device (the reference re-allocates three byte arenas per call,
    DGR/rasterize_points.cu:73-78)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    h = _HANDLES.get(idx)
    if h is None:
        h = _HANDLES[idx] = Rasterizer(idx)
    return h


class GaussianRasterizationSettings(NamedTuple):
    """DGR/diff_gaussian_rasterization/__init__.py:157-169."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _none_if_empty(t):
    return None if t is None or t.numel() == 0 else _f32c(t)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    """DGR __init__.py:21-44.  Gradients wanted: the autograd Function; otherwise the plain forward."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (
            means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)):
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                         raster_settings)
    return _rasterize_no_grad(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


def _rasterize_no_grad(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """_RasterizeGaussians.forward (DGR __init__.py:46-98) without a graph."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")   # rasterize_points.cu:57-59
    rs = raster_settings
    h = _handle(means3D.device)
    if rs.debug:
        # the reference's debug mode (DGR __init__.py:83-90): keep a host copy of every argument and, if the rasteriser
        # fails, leave it in snapshot_fw.dump for post-mortem; the C ABI call itself runs with a sync + check per launch
        keep = tuple(t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t for t in (
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos,
            rs.prefiltered, rs.debug))
        try:
            return _forward(h, rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        except Exception as ex:
            torch.save(keep, "snapshot_fw.dump")
            print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise ex
    return _forward(h, rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)


def _call_args(rs, sh, colors_precomp, scales, rotations, cov3Ds_precomp):
    """What ``Rasterizer.forward`` and ``.backward`` both take after the per-Gaussian leading arguments: the camera tuple and
    the keyword arguments (an empty tensor = not given)."""
    cam = (_f32c(rs.viewmatrix), _f32c(rs.projmatrix), _f32c(rs.campos), _f32c(rs.bg), int(rs.image_width),
           int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy))
    args = dict(shs=_none_if_empty(sh), colors_precomp=_none_if_empty(colors_precomp), scales=_none_if_empty(scales),
                rotations=_none_if_empty(rotations), cov3D_precomp=_none_if_empty(cov3Ds_precomp), sh_degree=int(rs.sh_degree),
                scale_modifier=float(rs.scale_modifier), debug=bool(rs.debug))
    return cam, args


def _forward(h, rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
    cam, args = _call_args(rs, sh, colors_precomp, scales, rotations, cov3Ds_precomp)
    return h.forward(_f32c(means3D), _f32c(opacities).reshape(-1), *cam, prefiltered=bool(rs.prefiltered), **args)


def _function_forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """Forward of both autograd Functions: the plain forward, and in ``ctx`` the inputs, the handle and the handle's call count
    (the reference keeps its three byte arenas in ``ctx``; here the forward state lives in the per-device handle)."""
    color, radii = _rasterize_no_grad(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)
    h = _handle(means3D.device)
    ctx.raster_settings = raster_settings
    ctx.handle = h
    ctx.state_calls = h.state_calls
    ctx.opacity_shape = tuple(opacities.shape)
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh, opacities)
    ctx.mark_non_differentiable(radii)
    return h, color, radii


def _function_backward(ctx, grad_color, ray_depth=False, **map_grads):
    """Backward of the autograd Functions (``ray_depth``: the maps are the ray maps, ``Rasterizer.backward(ray_depth=True)``): one ``Rasterizer.backward`` call with the upstream gradient of the image and, for the
    depth Function, of the maps (``grad_depth`` / ``grad_median`` / ``grad_alpha``).  If another forward (or ``render_views``)
    has overwritten the handle's state since ours -- two forwards before one backward, several views per optimiser step, another
    user of the handle -- ours is replayed first into a scratch image.  With ``raster_settings.debug`` a failure leaves the
    arguments in ``snapshot_bw.dump`` (the reference's debug mode, DGR __init__.py:118-132), for the depth Function too.
    -> the nine gradients of DGR __init__.py:143-153."""
    rs = ctx.raster_settings
    h = ctx.handle
    colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh, opacities = ctx.saved_tensors
    cam, args = _call_args(rs, sh, colors_precomp, scales, rotations, cov3Ds_precomp)
    opt = lambda t: None if t is None else _f32c(t)   # an output the loss does not use: a NULL map

    def run():
        if h.state_calls != ctx.state_calls:
            h.forward(_f32c(means3D), _f32c(opacities).reshape(-1), *cam, prefiltered=bool(rs.prefiltered), **args)
            ctx.state_calls = h.state_calls
        more = dict(ray_depth=True) if ray_depth else {}
        return h.backward(opt(grad_color), _f32c(means3D), *cam, **{k: opt(v) for k, v in map_grads.items()}, **more, **args)

    if rs.debug:
        keep = tuple(t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t for t in (
            rs.bg, means3D, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_color, sh, rs.sh_degree, rs.campos, rs.debug))
        try:
            g = run()
        except Exception as ex:
            torch.save(keep, "snapshot_bw.dump")
            print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise ex
    else:
        g = run()
    given = lambda t: t is not None and t.numel() > 0
    # means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings
    return (g["mean3D"], g["mean2D"], g["sh"] if given(sh) else None, g["color"] if given(colors_precomp) else None,
            g["opacity"].reshape(ctx.opacity_shape), g["scale"] if given(scales) else None,
            g["rot"] if given(rotations) else None, g["cov3D"] if given(cov3Ds_precomp) else None, None)


class _RasterizeGaussians(torch.autograd.Function):
    """DGR __init__.py:44-155: ``(color, radii)`` out, nine gradients back (``_function_forward`` / ``_function_backward``)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        _, color, radii = _function_forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                            raster_settings)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _):
        return _function_backward(ctx, grad_out_color)


class _RasterizeGaussiansDepth(torch.autograd.Function):
    """``_RasterizeGaussians`` with the depth and opacity maps as three more differentiable outputs (an extension).  The
    backward passes the four upstream gradients to one ``Rasterizer.backward`` call (``gs2m_rasterize_backward_depth``); an
    output the loss does not use arrives as None and is passed as a NULL map.  Everything else -- the replay when the handle's
    state has moved on, the ``debug`` snapshot, the gradient tuple -- is the colour Function's, by the same code."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        h, color, radii = _function_forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                            raster_settings)
        maps = h.depth_maps(int(raster_settings.image_width), int(raster_settings.image_height), like=color)
        ctx.set_materialize_grads(False)
        return color, radii, maps["expected"], maps["median"], maps["alpha"]

    @staticmethod
    def backward(ctx, grad_color, _, grad_expected, grad_median, grad_alpha):
        if grad_color is None and grad_expected is None and grad_median is None and grad_alpha is None:
            rs = ctx.raster_settings
            grad_color = torch.zeros((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32,
                                     device=ctx.saved_tensors[1].device)
        return _function_backward(ctx, grad_color, grad_depth=grad_expected, grad_median=grad_median, grad_alpha=grad_alpha)


class _RasterizeGaussiansRayDepth(torch.autograd.Function):
    """``_RasterizeGaussiansDepth`` with the RAY maps: ``expected`` and ``median`` are those of ``depth_maps_ray`` (the depth at
    which the pixel's ray meets each contributing Gaussian) and the backward is ``gs2m_rasterize_backward_depth_ray``, through
    which a depth loss reaches rotations and scales by the geometry of the intersection.  Needs scales and rotations."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        rs = raster_settings
        h, color, radii = _function_forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs)
        maps = h.depth_maps_ray(_f32c(means3D), _f32c(scales), _f32c(rotations), _f32c(rs.viewmatrix), int(rs.image_width),
                                int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy),
                                scale_modifier=float(rs.scale_modifier), like=color)
        ctx.set_materialize_grads(False)
        return color, radii, maps["expected"], maps["median"], maps["alpha"]

    @staticmethod
    def backward(ctx, grad_color, _, grad_expected, grad_median, grad_alpha):
        if grad_color is None and grad_expected is None and grad_median is None and grad_alpha is None:
            rs = ctx.raster_settings
            grad_color = torch.zeros((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32,
                                     device=ctx.saved_tensors[1].device)
        return _function_backward(ctx, grad_color, ray_depth=True, grad_depth=grad_expected, grad_median=grad_median,
                                  grad_alpha=grad_alpha)


class GaussianRasterizer(nn.Module):
    """DGR/diff_gaussian_rasterization/__init__.py:171-220."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        self._last = None    # what depth_maps() needs of the last forward: its inputs, the handle and the handle's call count

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            rs = self.raster_settings
            h = _handle(positions.device)
            present = h.mark_visible(_f32c(positions), _f32c(rs.viewmatrix), _f32c(rs.projmatrix))
        return present.to(torch.bool)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, return_depth=False, ray_depth=False):
        """``return_depth=True`` (an extension; the reference returns ``(color, radii)``): ``(color, radii, expected, median,
        alpha)`` with the [H,W] maps of ``depth_maps``, carrying the graph when gradients are wanted.  With ``ray_depth=True``
        as well the two depth maps are ``expected_ray`` and ``median_ray`` (``gs2m_rasterize_depth_ray``; scales and rotations
        required) and their graph is ``gs2m_rasterize_backward_depth_ray``."""
        raster_settings = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])
        if ray_depth and not return_depth:
            raise ValueError("ray_depth=True selects the maps of return_depth=True")
        if ray_depth and (scales.numel() == 0 or rotations.numel() == 0):
            raise ValueError("ray_depth=True needs scales and rotations: a forward with cov3D_precomp has no ray depth")
        # Invoke the HIP rasterization routine
        tensors = (means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        with_graph = return_depth and torch.is_grad_enabled() and any(
            isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)
        if with_graph:
            out = (_RasterizeGaussiansRayDepth if ray_depth else _RasterizeGaussiansDepth).apply(*tensors, raster_settings)
        else:
            out = rasterize_gaussians(*tensors, raster_settings)
        h = _handle(means3D.device)
        self._last = (h, h.state_calls, tensors[:1] + tensors[2:])
        if return_depth and not with_graph:
            if ray_depth:
                maps = self.depth_maps(("expected_ray", "median_ray", "alpha"))
                out = (*out, maps["expected_ray"], maps["median_ray"], maps["alpha"])
            else:
                maps = self.depth_maps()
                out = (*out, maps["expected"], maps["median"], maps["alpha"])
        return out

    def depth_maps(self, want=("expected", "median", "alpha")):
        """Extension (the reference has no depth output): maps of THIS rasteriser's last ``forward`` as a dict of [H,W] float32
        tensors -- ``expected`` (alpha-weighted mean view-space z of the contributing Gaussians' centres), ``median`` (z of the
        contributor that takes the transmittance to 0.5 or below) and ``alpha`` (accumulated opacity); 0 = no contributor
        (``gs2m_rasterize_depth``).  If another forward ran on the device's handle since, this one is replayed first into a
        scratch image, the way the backward pass does.  The results are DETACHED; maps that carry the graph come from
        ``forward(..., return_depth=True)``.

        ``expected_ray`` and ``median_ray`` are the same two maps with the depth at which the pixel's ray meets each
        contributing Gaussian in place of its centre's z (``gs2m_rasterize_depth_ray``: one more call, from the inputs of the
        last forward).  They need ``scales`` and ``rotations``: after a forward with ``cov3D_precomp`` asking for them raises
        ``ValueError``.  Detached like the others; ray maps that carry the graph come from
        ``forward(..., return_depth=True, ray_depth=True)``."""
        names = ("expected", "median", "alpha")
        ray_names = {"expected_ray": "expected", "median_ray": "median"}
        if self._last is None:
            raise RuntimeError("GaussianRasterizer.depth_maps: this rasteriser has not run a forward")
        unknown = [w for w in want if w not in names and w not in ray_names]
        if unknown:
            raise ValueError(f"depth_maps: unknown map(s) {unknown}; known: {names + tuple(ray_names)}")
        h, calls, inputs = self._last
        rs = self.raster_settings
        means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp = inputs
        want_ray = tuple(ray_names[w] for w in ray_names if w in want)
        if want_ray and (scales.numel() == 0 or rotations.numel() == 0):
            raise ValueError("GaussianRasterizer.depth_maps: expected_ray / median_ray need scales and rotations; the last "
                             "forward took cov3D_precomp, which has no ray depth")
        with torch.no_grad():
            if h.state_calls != calls:
                _forward(h, rs, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
                self._last = (h, h.state_calls, inputs)
            W, H = int(rs.image_width), int(rs.image_height)
            out = h.depth_maps(W, H, want=tuple(w for w in want if w in names), like=_f32c(rs.bg)) \
                if any(w in names for w in want) else {}
            if want_ray:
                ray = h.depth_maps_ray(_f32c(means3D), _f32c(scales), _f32c(rotations), _f32c(rs.viewmatrix), W, H,
                                       float(rs.tanfovx), float(rs.tanfovy), scale_modifier=float(rs.scale_modifier),
                                       want=want_ray, like=_f32c(rs.bg))
                out.update({w: ray[k] for w, k in ray_names.items() if w in want})
            return out
