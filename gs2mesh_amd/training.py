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
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.random_background = False
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


def train(gaussians, cameras, images, opt, *, extent, bg, white_background=False, seed=0, callback=None, timing=None):
    """The loop of train.py:51-128 over ``opt.iterations`` iterations -> the loss of every iteration.

    ``gaussians``: a ``GaussianModel`` after ``training_setup(opt)``; ``cameras``: ``graphics.Camera`` objects; ``images``: the
    [3,H,W] ground truth of each, in [0,1], on the device; ``extent``: ``cameras_extent(cameras)``; ``bg``: [3] background on
    the device.  ``seed`` drives the choice of views (a stack refilled when empty, popped at random) and the random
    background.  ``callback(iteration, event, gaussians, counts)`` is called after every densification (``"densify"``, with the
    ``{"cloned", "split", "pruned"}`` counts of ``densify_and_prune``) and opacity reset (``"reset_opacity"``, None).  ``timing``: None, or a dict that receives the stream time in ms of the four phases of
    every iteration (lists under ``render``, ``loss``, ``backward``, ``update``), measured with events and read at the end."""
    from .gaussian_renderer import render
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
        pkg = render(cameras[view], gaussians, pipe, background)
        image, viewspace, visible, radii = pkg["render"], pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"]
        if t:
            t.append(mark())
        loss = loss_fn(image, images[view], opt.lambda_dssim)
        if t:
            t.append(mark())
        loss.backward()
        if t:
            t.append(mark())
        with torch.no_grad():
            losses.append(loss.detach())
            if iteration < opt.densify_until_iter:
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
