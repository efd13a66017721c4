"""A splat on a ring of cameras as the part of ``Renderer`` that ``RenderedDepth`` and ``TSDF`` read: the scene of
tests/test_rendered_depth*.py.  Not collected by pytest."""
from argparse import Namespace

import numpy as np
import torch

from gs2mesh_amd import synthetic
from gs2mesh_amd.gaussian_model import GaussianModel

SPHERE_RADIUS, RING_RADIUS, BASELINE = 0.6, 3.5, 0.245


class SplatScene(synthetic.DiskScene):
    """``synthetic.textured_sphere`` (opaque isotropic splats on a sphere of radius 0.6) seen from ``n_views`` ring cameras;
    ``left_view`` is the accessor ``Renderer`` has."""

    def __init__(self, root, n_views, W, H, focal, P, device, seed=7, sigma=0.03, bg=(0.0, 0.0, 0.0)):
        self.poses = synthetic.ring_poses(n_views, RING_RADIUS)
        super().__init__(str(root), self.poses, W, H, focal, BASELINE)
        self.arrays = synthetic.textured_sphere(P, seed, SPHERE_RADIUS, sigma)
        self.gaussians = GaussianModel(3, device=device)
        g = self.arrays
        self.gaussians.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
        self.background = torch.tensor(bg, dtype=torch.float32, device=device)
        self.W, self.H, self.focal = W, H, focal

    def camera(self, i):
        return synthetic.stereo_cameras(self.poses[i], self.W, self.H, self.focal, self.focal, BASELINE)[0]

    def left_view(self, i):
        return self.camera(i), self.gaussians, self.background


def tsdf_args(**kw):
    """the TSDF arguments of the scene: 1/64 voxels, truncation 0.1, depths between 4 and 20 baselines (0.98 .. 4.9)"""
    a = dict(TSDF_scale=1.0, TSDF_dilate=1, TSDF_valid=None, TSDF_skip=None, TSDF_use_occlusion_mask=True, TSDF_use_mask=False,
             TSDF_invert_mask=False, TSDF_erode_mask=True, TSDF_erosion_kernel_size=10, TSDF_closing_kernel_size=10, TSDF_voxel=8,
             TSDF_sdf_trunc=0.1, TSDF_min_depth_baselines=4, TSDF_max_depth_baselines=20, TSDF_cleaning_threshold=100000)
    a.update(kw)
    return Namespace(**a)


def sphere_hit(scene, i):
    """[H,W] bool: the pixel's ray meets the sphere"""
    c = scene.left_cameras[i]
    return synthetic.sphere_depth(scene.poses[i], c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], SPHERE_RADIUS) > 0


def np_of(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
