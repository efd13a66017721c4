"""3DGS training on the HIP rasteriser: the losses (GS/utils/loss_utils.py), the optimisation defaults
(GS/arguments/__init__.py:71-90) and the loop of GS/train.py:51-128, restated on this package's ``GaussianModel``,
``render`` and ``graphics.Camera``.  Point cloud + posed images -> trained Gaussians; ``tools/train_splat.py`` is the
command-line front.  The loop uses the operator-level path (``diff_gaussian_rasterization``): the packed model and the
pair batch of ``render_views`` have no backward.  Importing this module needs neither a GPU nor the built library."""
from __future__ import annotations

import math
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import _empty, _is_torch, _ptr, _stream_of


def l1_loss(network_output, gt):
    """loss_utils.py:17-18"""
    return torch.abs(network_output - gt).mean()


def _window(window_size, channel, like):
    """loss_utils.py:23-31: normalised 1-D Gaussian (sigma 1.5), its outer product, one copy per channel"""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w.expand(channel, 1, window_size, window_size).contiguous().to(device=like.device, dtype=like.dtype)


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.py:33-64: mean structural similarity over an 11 x 11 Gaussian window, zero padding, per channel
    (grouped conv2d); C1 = 0.01^2, C2 = 0.03^2.  ``img``: [3,H,W] or [B,3,H,W]."""
    channel = img1.size(-3)
    w = _window(window_size, channel, img1)
    conv = lambda x: F.conv2d(x, w, padding=window_size // 2, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


class OptimizationParams:
    """The reference's optimisation defaults (arguments/__init__.py:71-90) as plain attributes; keyword arguments override."""

    def __init__(self, **overrides):
        self.iterations = 30_000
        self.position_lr_init = 0.00016
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.feature_lr = 0.0025
        self.opacity_lr = 0.05
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.percent_dense = 0.01
        self.lambda_dssim = 0.2
        self.lambda_depth = 0.0             # weight of depth_l1_loss against train(..., depth_priors=...); an extension
        self.depth_kind = "centre"          # the rendered depth that loss compares: "centre" (z of the centres) or "ray" (the
                                            # ray-Gaussian intersection depth, whose gradient also turns the Gaussians)
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.random_background = False
        self.optimizer_type = "default"     # "fused" / "sparse_adam": optim.FusedAdam, dense or on the visible rows only
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise TypeError(f"OptimizationParams has no parameter {k!r}")
            setattr(self, k, v)


class PipelineParams:
    """arguments/__init__.py:63-69"""
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False


def cameras_extent(cameras):
    """The radius of getNerfppNorm (scene/dataset_readers.py:45-66): 1.1 x the largest distance of a camera centre from the
    mean centre.  It scales the position learning rate and the size thresholds of densification."""
    c = np.stack([np.asarray(cam.camera_center, np.float64) for cam in cameras])
    return float(1.1 * np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max())


def loss_fn(image, gt, lambda_dssim):
    """train.py:89-90"""
    return (1.0 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1.0 - ssim(image, gt))


def depth_l1_loss(depth, alpha, prior, valid=None):
    """Mean absolute difference between the rendered expected depth (``render(..., return_depth=True, depth_grad=True)["depth"]``)
    and a prior depth map over ``valid & (prior > 0)``: 0 in ``prior`` means "no depth", as everywhere in the package.  The
    rendered depth is detached nowhere, so the loss trains the splat through ``gs2m_rasterize_backward_depth``.  ``alpha`` is
    the rendered opacity map of the same call; this loss does not weight by it (the expected depth is already normalised by
    the accumulated weights) -- it is part of the signature so that coverage-weighted variants are drop-ins.  An empty mask
    gives a zero that still belongs to the graph."""
    mask = prior > 0
    if valid is not None:
        mask = mask & valid.to(torch.bool)
    n = mask.sum()
    diff = torch.where(mask, (depth - prior).abs(), torch.zeros_like(depth))
    return diff.sum() / n.clamp_min(1).to(depth.dtype)


# ---- the fused loss: gs2m_photo_loss_forward / _backward (gs2mesh_amd/csrc/loss_kernels.h) -----------------------------------
def _loss_planes(image, gt, what):
    if tuple(image.shape) != tuple(gt.shape) or image.ndim not in (3, 4):
        raise ValueError(f"{what}: image and target must be [C,H,W] or [B,C,H,W] of one shape, got {tuple(image.shape)} and "
                         f"{tuple(gt.shape)}")
    f32 = torch.float32 if _is_torch(image) else np.float32
    if image.dtype != f32 or gt.dtype != f32:
        raise TypeError(f"{what}: image and target must be float32, got {image.dtype} and {gt.dtype}")
    H, W = int(image.shape[-2]), int(image.shape[-1])
    return int(np.prod(image.shape[:-2], dtype=np.int64)), H, W


def photo_loss_forward(image, gt, lambda_dssim, want_partials=True, want_map=False, lib=None, stream=None):
    """``gs2m_photo_loss_forward`` on contiguous f32 device tensors (numpy arrays on the emulator back-end of the tests).
    -> (out [3] = loss, mean |x - y|, mean SSIM; partials [3,*image.shape] or None; the SSIM map or None).  Asynchronous on
    the stream; the scratch is kept per device (shared by every stream of it: order the calls on one) and only grows."""
    lib = lib or _lib.get()
    planes, H, W = _loss_planes(image, gt, "photo_loss_forward")
    if planes * H * W == 0:
        raise ValueError("photo_loss_forward: empty image")
    need = int(lib.gs2m_photo_loss_scratch_bytes(planes, H, W))
    if need < 0:
        raise ValueError(f"photo_loss_forward: unsupported size {tuple(image.shape)}")
    scratch = _lib.scratch("photo_loss", image, need)
    out = _empty(image, (3,), np.float32)
    partials = _empty(image, (3,) + tuple(image.shape), np.float32) if want_partials else None
    tap = _empty(image, tuple(image.shape), np.float32) if want_map else None
    _lib.check(lib.gs2m_photo_loss_forward(planes, H, W, _ptr(image, None, "image"), _ptr(gt, None, "target"), float(lambda_dssim),
                                           _ptr(scratch), scratch.shape[0] * 8, _ptr(out), _ptr(partials), _ptr(tap),
                                           _stream_of(image, stream)), lib)
    return out, partials, tap


def photo_loss_backward(image, gt, partials, lambda_dssim, grad_loss, lib=None, stream=None):
    """``gs2m_photo_loss_backward``: ``grad_loss`` is a one-element f32 buffer on the device (never read on the host).
    -> dL/d image, of ``image``'s shape."""
    lib = lib or _lib.get()
    planes, H, W = _loss_planes(image, gt, "photo_loss_backward")
    if tuple(partials.shape) != (3,) + tuple(image.shape):
        raise ValueError(f"photo_loss_backward: partials must be {(3,) + tuple(image.shape)}, got {tuple(partials.shape)}")
    if int(np.prod(grad_loss.shape, dtype=np.int64)) != 1:
        raise ValueError(f"photo_loss_backward: grad_loss must hold one element, got {tuple(grad_loss.shape)}")
    grad = _empty(image, tuple(image.shape), np.float32)
    _lib.check(lib.gs2m_photo_loss_backward(planes, H, W, _ptr(image, None, "image"), _ptr(gt, None, "target"),
                                            _ptr(partials, None, "partials"), float(lambda_dssim),
                                            _ptr(grad_loss, None, "grad_loss"), _ptr(grad), _stream_of(image, stream)), lib)
    return grad


class _FusedLoss(torch.autograd.Function):
    """out[which] of the forward kernel; the backward kernel with autograd's incoming gradient as its device scalar"""

    @staticmethod
    def forward(ctx, image, gt, lambda_dssim, which, need_grad, lib):
        out, partials, _ = photo_loss_forward(image, gt, lambda_dssim, want_partials=need_grad, lib=lib)
        if need_grad:
            ctx.save_for_backward(image, gt, partials)
        ctx.args = (lambda_dssim, which, lib)
        return out[which]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        image, gt, partials = ctx.saved_tensors
        lambda_dssim, which, lib = ctx.args
        g = grad_output.to(torch.float32).reshape(1).contiguous()
        if which == 2:                      # mean SSIM = 1 - loss at lambda = 1
            g = -g
        return photo_loss_backward(image, gt, partials, lambda_dssim, g, lib=lib), None, None, None, None, None


def _fused(image, gt, lambda_dssim, which, lib, what):
    if not _is_torch(image):                # the emulator back-end of the tests: the value alone, no graph
        return photo_loss_forward(np.ascontiguousarray(image), np.ascontiguousarray(gt), lambda_dssim, want_partials=False,
                                  lib=lib)[0][which]
    if not _is_torch(gt):
        raise TypeError(f"{what}: the target must be a torch tensor like the image")
    if gt.requires_grad:
        raise RuntimeError(f"{what}: no gradient is computed for the target; detach it")
    _loss_planes(image, gt, what)
    image = image.contiguous()              # the one copy of a non-contiguous render; autograd carries the gradient back
    _lib.MEMORY.ptr(image.detach(), torch.float32, "image")                 # a CPU tensor is an error, before any work
    need_grad = torch.is_grad_enabled() and image.requires_grad
    return _FusedLoss.apply(image, gt.contiguous(), float(lambda_dssim), which, need_grad, lib)


def fused_loss(image, gt, lambda_dssim, *, lib=None):
    """``loss_fn`` on the HIP kernels of ``gs2m_photo_loss_forward`` / ``_backward`` (include/gs2mesh_amd.h states the
    arithmetic and how far it is from ``loss_fn``): a 0-d tensor, differentiable in ``image``.  ``image``, ``gt``: f32 on the HIP
    device, [3,H,W], [C,H,W] or [B,C,H,W] (the leading dimensions are planes).  Window 11 only; a ``gt`` that requires grad
    raises.  The partial derivatives are written only when ``image`` requires grad.  There is no double backward.  The
    scratch of the tile sums is one buffer per device: calls on one device must be ordered on one stream (two streams
    calling concurrently would race on it, as with ``simple_knn``'s scratch)."""
    return _fused(image, gt, lambda_dssim, 0, lib, "fused_loss")


def fused_ssim(img1, img2, *, lib=None):
    """The mean of ``ssim(img1, img2)`` through the same kernels, differentiable in ``img1``: the drop-in for code that
    calls ``ssim(a, b)`` on its own.  It takes the two images only (window 11, the mean): a third positional argument, as in
    ``ssim(a, b, 11)``, is a TypeError.  One scratch buffer per device, as ``fused_loss``."""
    return _fused(img1, img2, 1.0, 2, lib, "fused_ssim")


def train(gaussians, cameras, images, opt, *, extent, bg, white_background=False, seed=0, callback=None, timing=None,
          loss="torch", depth_priors=None):
    """The loop of train.py:51-128 over ``opt.iterations`` iterations -> the loss of every iteration.

    ``gaussians``: a ``GaussianModel`` after ``training_setup(opt)``; ``cameras``: ``graphics.Camera`` objects; ``images``: the
    [3,H,W] ground truth of each, in [0,1], on the device; ``extent``: ``cameras_extent(cameras)``; ``bg``: [3] background on
    the device.  ``seed`` drives the choice of views (a stack refilled when empty, popped at random) and the random
    background.  ``callback(iteration, event, gaussians, counts)`` is called after every densification (``"densify"``, with the
    ``{"cloned", "split", "pruned"}`` counts of ``densify_and_prune``) and opacity reset (``"reset_opacity"``, None).  ``timing``: None, or a dict that receives the stream time in ms of the four phases of
    every iteration (lists under ``render``, ``loss``, ``backward``, ``update``), measured with events and read at the end.
    ``loss``: ``"torch"`` (``loss_fn``, the default) or ``"fused"`` (``fused_loss``, the HIP kernels).  With
    ``opt.optimizer_type`` ``"fused"`` or ``"sparse_adam"`` (``gaussians.optimizer`` is then an ``optim.FusedAdam``) the
    densification statistics and the step are one kernel each, and an iteration that neither densifies nor resets opacity
    has no host wait in its update phase; ``"sparse_adam"`` steps only the rows the view saw (``radii > 0``).
    ``depth_priors``: None, or one [H,W] depth map per camera on the device (view-space z, 0 = invalid; e.g. what ``Stereo`` or
    ``RenderedDepth`` wrote).  With priors and ``opt.lambda_depth > 0`` every iteration renders with ``depth_grad=True`` and adds
    ``opt.lambda_depth * depth_l1_loss(depth, alpha, prior)`` to its loss; otherwise the loop is unchanged.  ``opt.depth_kind``
    chooses that depth: ``"centre"`` (the default: ``pkg["depth"]``, through ``gs2m_rasterize_backward_depth``) or ``"ray"``
    (``pkg["ray_depth"]`` of ``render(..., ray_depth=True)``, through ``gs2m_rasterize_backward_depth_ray``)."""
    if loss not in ("torch", "fused"):
        raise ValueError(f"train: loss must be 'torch' or 'fused', got {loss!r}")
    lambda_depth = float(getattr(opt, "lambda_depth", 0.0)) if depth_priors is not None else 0.0
    if lambda_depth > 0.0 and len(depth_priors) != len(cameras):
        raise ValueError(f"train: {len(depth_priors)} depth priors for {len(cameras)} cameras")
    depth_kind = getattr(opt, "depth_kind", "centre")
    if depth_kind not in ("centre", "ray"):
        raise ValueError(f"train: opt.depth_kind must be 'centre' or 'ray', got {depth_kind!r}")
    from .gaussian_renderer import render
    loss_of = fused_loss if loss == "fused" else loss_fn
    from .optim import FusedAdam
    native_update = isinstance(gaussians.optimizer, FusedAdam)
    sparse = native_update and getattr(opt, "optimizer_type", "default") == "sparse_adam"
    rng = random.Random(seed)
    pipe = PipelineParams()
    losses = []
    stack = []
    stamps = []
    mark = None
    if timing is not None:
        def mark():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e
    for iteration in range(1, opt.iterations + 1):
        t = [mark()] if mark else None
        gaussians.update_learning_rate(iteration)
        if iteration % 1000 == 0:
            gaussians.oneupSHdegree()
        if not stack:
            stack = list(range(len(cameras)))
        view = stack.pop(rng.randint(0, len(stack) - 1))
        background = bg
        if opt.random_background:
            background = torch.tensor([rng.random() for _ in range(3)], dtype=torch.float32, device=bg.device)
        if lambda_depth > 0.0:
            pkg = render(cameras[view], gaussians, pipe, background, return_depth=True, depth_grad=True,
                         ray_depth=depth_kind == "ray")
        else:
            pkg = render(cameras[view], gaussians, pipe, background)
        image, viewspace, visible, radii = pkg["render"], pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"]
        if t:
            t.append(mark())
        loss = loss_of(image, images[view], opt.lambda_dssim)
        if lambda_depth > 0.0:
            loss = loss + lambda_depth * depth_l1_loss(pkg["ray_depth" if depth_kind == "ray" else "depth"], pkg["alpha"], depth_priors[view])
        if t:
            t.append(mark())
        loss.backward()
        if t:
            t.append(mark())
        with torch.no_grad():
            losses.append(loss.detach())
            if iteration < opt.densify_until_iter:
                if native_update:
                    gaussians.update_densification_stats(viewspace, radii)
                else:
                    gaussians.max_radii2D[visible] = torch.max(gaussians.max_radii2D[visible], radii[visible].to(gaussians.max_radii2D.dtype))
                    gaussians.add_densification_stats(viewspace, visible)
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                    counts = gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, extent, size_threshold)
                    if callback:
                        callback(iteration, "densify", gaussians, counts)
                if iteration % opt.opacity_reset_interval == 0 or (white_background and iteration == opt.densify_from_iter):
                    gaussians.reset_opacity()
                    if callback:
                        callback(iteration, "reset_opacity", gaussians, None)
            if iteration < opt.iterations:
                if native_update:
                    gaussians.optimizer.step(visible=radii if sparse else None)
                else:
                    gaussians.optimizer.step()
                gaussians.optimizer.zero_grad(set_to_none=True)
        if t:
            t.append(mark())
            stamps.append(t)
    if timing is not None:
        torch.cuda.synchronize()
        for k, name in enumerate(("render", "loss", "backward", "update")):
            timing[name] = [s[k].elapsed_time(s[k + 1]) for s in stamps]
    return [float(x) for x in torch.stack(losses).tolist()] if losses else []


def synthetic_scene(device, n_true=1500, n_init=300, n_views=6, width=96, height=80, focal=165.0, seed=0, ring_radius=3.5):
    """A training problem that needs no dataset: ground truth = ``synthetic.textured_sphere`` rendered (under ``no_grad``)
    from ``n_views`` cameras on the ring of ``synthetic.ring_poses``; initial cloud = ``n_init`` of the true centres with their
    DC colours.  -> (cameras, images, BasicPointCloud, the ground-truth GaussianModel, black background [3])."""
    from . import synthetic
    from .gaussian_model import GaussianModel
    from .gaussian_renderer import render
    from .graphics import BasicPointCloud, Camera, focal2fov
    from .sh_utils import SH2RGB
    g = synthetic.textured_sphere(n_true, seed)
    truth = GaussianModel(3, device=device)
    truth.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    cameras = [Camera(i, p[:, :3].T, p[:, 3], focal2fov(focal, width), focal2fov(focal, height), width, height, uid=i)
               for i, p in enumerate(synthetic.ring_poses(n_views, ring_radius))]
    bg = torch.zeros(3, dtype=torch.float32, device=device)
    with torch.no_grad():
        images = [render(c, truth, PipelineParams(), bg)["render"].clamp(0, 1).clone() for c in cameras]
    pick = np.random.default_rng(seed + 1).choice(n_true, size=n_init, replace=False)
    pcd = BasicPointCloud(points=g["xyz"][pick], colors=np.clip(SH2RGB(g["features_dc"][pick, 0, :]), 0, 1),
                          normals=np.zeros((n_init, 3), np.float32))
    return cameras, images, pcd, truth, bg
