"""``render()`` with the reference's signature and return dict (GS/gaussian_renderer/__init__.py:18-100),
on the HIP rasteriser.  For callers that hold a 3DGS ``Camera``-like object and a ``GaussianModel``: the training loop
(``gs2mesh_amd.training``) and anything written against the reference's ``render``; the pipeline class ``Renderer`` uses the
fused stereo entry point instead.  Under ``torch.no_grad()``, or with a model whose tensors do not require grad (``load_ply`` /
``load_arrays``), it is the plain forward; otherwise the rasteriser records the graph and ``viewspace_points`` carries the
screen-space gradient densification reads."""
from __future__ import annotations

import math

import torch

from .diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer


def _dev(x, device):
    return torch.as_tensor(x, dtype=torch.float32, device=device).contiguous()


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, return_depth=False,
           depth_grad=False, ray_depth=False):
    """Background tensor (bg_color) must be on the GPU, as in the reference.  ``return_depth=True`` (an extension: the reference
    renders colour only) adds three [H,W] maps of the same forward to the dict: ``depth`` (alpha-weighted mean
    view-space z of the contributing Gaussians' centres), ``median_depth`` (z of the contributor that takes the transmittance
    to one half) and ``alpha`` (accumulated opacity; render = C + (1 - alpha) * bg); 0 = no contributor.  They are detached
    unless ``depth_grad=True``: then, where gradients are wanted, they carry the graph (``gs2m_rasterize_backward_depth``) and
    a loss on them trains the splat; ``viewspace_points.grad`` then includes their screen-space term.
    ``ray_depth=True`` (with ``return_depth``) adds ``ray_depth`` and ``ray_median_depth``: the same two depth maps with the
    depth at which the pixel's ray meets each contributing Gaussian in place of its centre's z (``gs2m_rasterize_depth_ray``) --
    the plane of a flat Gaussian instead of a staircase.  With ``depth_grad=False`` these two are detached like the others.  With
    ``depth_grad=True``, where gradients are wanted, THEY carry the graph (``gs2m_rasterize_backward_depth_ray``): a loss on them
    reaches rotations and scales through the geometry of the intersection, which a loss on ``depth`` cannot; ``alpha`` carries
    the graph as before, and ``depth`` / ``median_depth`` are then detached (one backward pass per forward).  Not available
    with ``pipe.compute_cov3D_python``."""
    device = pc.get_xyz.device
    tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
    tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=tanfovx, tanfovy=tanfovy, bg=_dev(bg_color, device), scale_modifier=scaling_modifier,
        viewmatrix=_dev(viewpoint_camera.world_view_transform, device),
        projmatrix=_dev(viewpoint_camera.full_proj_transform, device), sh_degree=pc.active_sh_degree,
        campos=_dev(viewpoint_camera.camera_center, device), prefiltered=False,
        debug=bool(getattr(pipe, "debug", False)))
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)
    # 3D covariance: from scale / rotation inside the rasteriser, or (pipe.compute_cov3D_python, :56-61) on the host side
    scales = rotations = cov3D_precomp = None
    if getattr(pipe, "compute_cov3D_python", False):
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales = pc.get_scaling
        rotations = pc.get_rotation
    # colour: SH evaluated by the rasteriser, or (pipe.convert_SHs_python, :67-78) in torch, or the caller's override
    shs = colors_precomp = None
    if override_color is None:
        if getattr(pipe, "convert_SHs_python", False):
            from .sh_utils import eval_sh
            n_coef = (pc.max_sh_degree + 1) ** 2
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, n_coef)
            dir_pp = pc.get_xyz - _dev(viewpoint_camera.camera_center, device).repeat(pc.get_features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized) + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color
    means3D, opacity = pc.get_xyz, pc.get_opacity
    want_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (means3D, opacity, shs, colors_precomp, scales, rotations, cov3D_precomp))
    if want_grad:
        # the reference's gradient carrier (:26-30): the rasteriser's backward leaves d loss / d (screen position) in its .grad,
        # which GaussianModel.add_densification_stats reads
        screenspace_points = torch.zeros_like(means3D, requires_grad=True)
        screenspace_points.retain_grad()
    else:
        screenspace_points = torch.zeros_like(means3D)
    inputs = dict(means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp, opacities=opacity,
                  scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    maps = ray = None
    with torch.enable_grad() if want_grad else torch.no_grad():
        if return_depth and depth_grad and want_grad and ray_depth:   # the ray maps and alpha are the Function's outputs
            rendered_image, radii, expected, median, alpha = rasterizer(**inputs, return_depth=True, ray_depth=True)
            ray = {"expected_ray": expected, "median_ray": median}
            maps = dict(rasterizer.depth_maps(want=("expected", "median")), alpha=alpha)
        elif return_depth and depth_grad and want_grad:   # the maps are outputs of the autograd Function: they carry the graph
            rendered_image, radii, expected, median, alpha = rasterizer(**inputs, return_depth=True)
            maps = {"expected": expected, "median": median, "alpha": alpha}
        else:
            rendered_image, radii = rasterizer(**inputs)
    out = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
           "radii": radii}
    if return_depth:
        if maps is None:
            maps = rasterizer.depth_maps()
        out.update(depth=maps["expected"], median_depth=maps["median"], alpha=maps["alpha"])
        if ray_depth:
            if ray is None:
                ray = rasterizer.depth_maps(want=("expected_ray", "median_ray"))
            out.update(ray_depth=ray["expected_ray"], ray_median_depth=ray["median_ray"])
    return out
