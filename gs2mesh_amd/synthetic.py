"""Synthetic workloads for BASELINE.json's configs.

There are no datasets or trained splats in the build/bench environment, so every
measurement and full-size parity property runs on seeded synthetic inputs of the named
shapes: ``synth_v1`` Gaussians, ring-of-cameras stereo poses, analytic sphere depth maps.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np

from .graphics import Camera

SH_C0 = 0.28209479177387814  # GS/utils/sh_utils.py:24


def RGB2SH(rgb):
    """GS/utils/sh_utils.py:114-115."""
    return (rgb - 0.5) / SH_C0


@dataclass
class Config:
    name: str
    P: int
    seed: int
    log_s_mu: float
    width: int
    height: int
    focal: float
    n_pairs: int
    baseline_pct: float
    tsdf_n: int          # "N^3" label
    tsdf_extent: float
    sdf_trunc: float
    sphere_radius: float
    ring_radius: float = 3.5

    @property
    def voxel_length(self):
        return self.tsdf_extent / self.tsdf_n

    @property
    def baseline(self):
        return self.ring_radius * self.baseline_pct / 100.0


# BASELINE.md section 3 / SURVEY.md 8(d)
CONFIGS = {
    "C1": Config("C1", 10_000, 1001, math.log(0.02), 400, 300, 400.0, 2, 7.0, 128, 2.0, 0.16, 0.6),
    "C2": Config("C2", 300_000, 1002, math.log(0.006), 1600, 1200, 2900.0, 49, 7.0, 512, 2.0, 0.04, 0.6),
    "C3": Config("C3", 2_000_000, 1003, math.log(0.004), 1280, 840, 1100.0, 200, 7.0, 512, 2.0, 0.04, 0.6),
    "C4": Config("C4", 2_500_000, 1004, math.log(0.004), 1920, 1080, 1150.0, 300, 7.0, 1024, 4.0, 0.04, 1.2),
    "C5": Config("C5", 500_000, 1005, math.log(0.006), 1920, 1440, 1500.0, 120, 14.0, 512, 2.0, 0.04, 0.6),
}


def synth_v1(P, seed, log_s_mu):
    """Pre-activation Gaussian parameters in GaussianModel layout (all float32):
    xyz[P,3], features_dc[P,1,3], features_rest[P,15,3], scaling[P,3] (log), rotation[P,4]
    (wxyz, unnormalised), opacity[P,1] (logit)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, size=(P, 3)).astype(np.float32)
    scaling = rng.normal(log_s_mu, 0.4, size=(P, 3)).astype(np.float32)
    rotation = rng.normal(0.0, 1.0, size=(P, 4)).astype(np.float32)
    o = rng.uniform(0.05, 0.95, size=(P, 1))
    opacity = np.log(o / (1.0 - o)).astype(np.float32)
    f_dc = RGB2SH(rng.uniform(0.0, 1.0, size=(P, 1, 3))).astype(np.float32)
    f_rest = rng.normal(0.0, 0.05, size=(P, 15, 3)).astype(np.float32)
    return dict(xyz=xyz, features_dc=f_dc, features_rest=f_rest, scaling=scaling, rotation=rotation,
                opacity=opacity)


def trained_like(P, seed, log_s_mu, focal=2900.0, ring_radius=3.5):
    """Gaussians with the statistics of a TRAINED splat that ``synth_v1`` lacks (same layout): strongly anisotropic
    scales (10-100 : 1, surface-aligned discs and needles), 30 % of the opacities saturated at sigmoid >= 0.985 (the
    reference's 0.99 alpha cap, forward.cu:343), a mass of near-transparent ones, 0.1 % background splats whose screen
    radius exceeds 300 px (hundreds of tiles each: the > 64-tile walk of the binning), most centres on a surface shell,
    duplicated centres (exact depth ties in every view) and SH rest coefficients large enough to clamp colours at 0."""
    rng = np.random.default_rng(seed)
    n_shell = int(0.7 * P)
    d = rng.normal(size=(n_shell, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = d * (0.6 + rng.normal(0.0, 0.01, size=(n_shell, 1)))
    xyz = np.concatenate([shell, rng.uniform(-1.0, 1.0, size=(P - n_shell, 3))]).astype(np.float32)
    n_dup = max(2, P // 50)                                   # exact depth ties: copies of other centres
    dst = rng.choice(P, n_dup, replace=False)
    xyz[dst] = xyz[rng.choice(P, n_dup)]
    scaling = rng.normal(log_s_mu, 0.5, size=(P, 3))
    thin = rng.integers(1, 3, size=P)                         # 1 thin axis = disc, 2 = needle
    ratio = np.log(rng.uniform(10.0, 100.0, size=P))
    for a in range(3):
        scaling[:, a] -= np.where((a < thin), ratio, 0.0)
    perm = np.argsort(rng.random((P, 3)), axis=1)             # which axes are the thin ones
    scaling = np.take_along_axis(scaling, perm, axis=1)
    n_big = max(1, P // 1000)                                 # background splats: radius = 3 sigma f / z > 300 px
    big = rng.choice(P, n_big, replace=False)
    sigma = rng.uniform(1.0, 2.0, size=n_big) * 300.0 * ring_radius / (3.0 * focal)
    scaling[big, 0] = np.log(sigma)
    scaling[big, 1] = np.log(sigma * rng.uniform(0.3, 1.0, size=n_big))
    scaling[big, 2] = np.log(sigma * 0.01)
    u = rng.random(P)
    o = np.where(u < 0.30, rng.uniform(0.985, 0.9997, size=P),
                 np.where(u < 0.60, rng.uniform(0.004, 0.1, size=P), rng.uniform(0.1, 0.98, size=P)))
    o[big] = rng.uniform(0.02, 0.3, size=n_big)
    opacity = np.log(o / (1.0 - o)).astype(np.float32).reshape(P, 1)
    rotation = rng.normal(0.0, 1.0, size=(P, 4)).astype(np.float32)
    f_dc = RGB2SH(rng.uniform(0.0, 1.0, size=(P, 1, 3))).astype(np.float32)
    f_rest = rng.normal(0.0, 0.15, size=(P, 15, 3)).astype(np.float32)
    return dict(xyz=xyz, features_dc=f_dc, features_rest=f_rest, scaling=scaling.astype(np.float32), rotation=rotation,
                opacity=opacity)


def ring_pose(azimuth, radius=3.5):
    """COLMAP world->camera [R|t] of a camera on a horizontal ring looking at the origin,
    up = -y (COLMAP: +x right, +y down, +z forward)."""
    c = np.array([radius * math.sin(azimuth), 0.0, -radius * math.cos(azimuth)])
    z = -c / np.linalg.norm(c)                 # forward: towards origin
    y = np.array([0.0, 1.0, 0.0])              # image-down = world +y  (up = -y)
    x = np.cross(y, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=0)            # rows = camera axes in world coords -> world->cam
    t = -R @ c
    return R, t


def ring_poses(n, radius=3.5, first=0, total=None):
    """n world->cam poses [n,3,4]; azimuths are k*2pi/total for k = first..first+n-1."""
    total = n if total is None else total
    out = np.zeros((n, 3, 4))
    for i in range(n):
        R, t = ring_pose(2.0 * math.pi * (first + i) / total, radius)
        out[i, :, :3] = R
        out[i, :, 3] = t
    return out


def stereo_cameras(pose_w2c, width, height, fx, fy, baseline):
    """(left, right) ``Camera`` for one COLMAP pose, exactly the pair Renderer.render_image_pair
    builds: R_gs = R_w2c^T, T_gs = t (left), T_gs = t - (baseline,0,0) (right)
    (verified against the reference's Euler detour in tests/test_golden_cameras.py)."""
    R = np.asarray(pose_w2c)[:, :3]
    t = np.asarray(pose_w2c)[:, 3]
    FoVx = 2 * np.arctan2(width, 2 * fx)
    FoVy = 2 * np.arctan2(height, 2 * fy)
    left = Camera(0, R.T, t, FoVx, FoVy, width, height)
    right = Camera(0, R.T, t - np.array([baseline, 0.0, 0.0]), FoVx, FoVy, width, height)
    return left, right


def sphere_depth(pose_w2c, width, height, fx, fy, cx, cy, radius):
    """Analytic z-depth map [H,W] float32 of a sphere of `radius` at the world origin
    (0 = no hit = invalid)."""
    R = np.asarray(pose_w2c)[:, :3]
    t = np.asarray(pose_w2c)[:, 3]
    u = (np.arange(width) - cx) / fx
    v = (np.arange(height) - cy) / fy
    dx, dy = np.meshgrid(u, v)
    d = np.stack([dx, dy, np.ones_like(dx)], axis=-1)          # camera-space ray, z = 1
    oc = t                                                      # sphere centre in camera coords = R*0 + t
    a = (d * d).sum(-1)
    b = -2.0 * (d @ oc)
    c = float(oc @ oc) - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
    s = np.where(s > 0, s, 0.0)
    return s.astype(np.float32)                                 # z-depth = s * d_z = s


def color_pattern(width, height):
    """Fixed u8 colour image ((u+v)%256, u%256, v%256)."""
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    return np.stack([(u + v) % 256, u % 256, v % 256], axis=-1).astype(np.uint8)


def sphere_depth_torch(pose_w2c, width, height, fx, fy, cx, cy, radius, device):
    """`sphere_depth` evaluated on the device (float64 maths, float32 result)."""
    import torch
    t = torch.as_tensor(np.asarray(pose_w2c)[:, 3], dtype=torch.float64, device=device)
    u = (torch.arange(width, dtype=torch.float64, device=device) - cx) / fx
    v = (torch.arange(height, dtype=torch.float64, device=device) - cy) / fy
    dy, dx = torch.meshgrid(v, u, indexing="ij")
    a = dx * dx + dy * dy + 1.0
    b = -2.0 * (dx * t[0] + dy * t[1] + t[2])
    c = float((t * t).sum()) - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = torch.where(hit, (-b - torch.sqrt(torch.clamp(disc, min=0.0))) / (2 * a), torch.zeros_like(a))
    s = torch.where(s > 0, s, torch.zeros_like(s))
    return s.to(torch.float32).contiguous()


class DiskScene:
    """The part of ``Renderer`` that ``TSDF`` reads (left cameras, baseline, render folders) for a scene written by
    ``write_tsdf_scene``."""

    def __init__(self, root, poses, width, height, focal, baseline):
        self.output_dir_root = root
        self.baseline = baseline
        self.left_cameras = []
        for p in poses:
            E = np.eye(4)
            E[:3] = p
            self.left_cameras.append(dict(width=width, height=height, fx=focal, fy=focal, cx=width / 2.0, cy=height / 2.0,
                                          extrinsic=np.linalg.inv(E)))

    def __len__(self):
        return len(self.left_cameras)

    def render_folder_name(self, i):
        return os.path.join(self.output_dir_root, f"{i:03}")


def write_tsdf_scene(root, n_views, width, height, focal, seed, model_name="DLNR_Middlebury", sphere_radius=0.6,
                     ring_radius=3.5, baseline_pct=7.0):
    """The on-disk layout ``TSDF.run`` reads for n_views views on a ring around a sphere: ``<root>/<i:03>/left.png`` (colour
    pattern), ``out_<model>/depth.npy`` (analytic sphere depth, seeded noise), ``left_mask.npy`` (the sphere's silhouette with
    seeded holes) and ``out_<model>/occlusion_mask.npy`` (seeded, ~5 % occluded).  Returns a ``DiskScene``."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    poses = ring_poses(n_views, ring_radius)
    scene = DiskScene(root, poses, width, height, focal, ring_radius * baseline_pct / 100.0)
    base = color_pattern(width, height)
    for i, p in enumerate(poses):
        d = scene.render_folder_name(i)
        os.makedirs(os.path.join(d, f"out_{model_name}"), exist_ok=True)
        depth = sphere_depth(p, width, height, focal, focal, width / 2.0, height / 2.0, sphere_radius)
        depth = depth + np.where(depth > 0, rng.normal(0.0, 1e-3, depth.shape), 0.0).astype(np.float32)
        mask = (depth > 0) & (rng.uniform(size=depth.shape) > 0.002)
        occ = rng.uniform(size=depth.shape) > 0.05
        Image.fromarray(np.roll(base, 7 * i, axis=1)).save(os.path.join(d, "left.png"), compress_level=1)
        np.save(os.path.join(d, f"out_{model_name}", "depth.npy"), depth.astype(np.float32))
        np.save(os.path.join(d, "left_mask.npy"), mask)
        np.save(os.path.join(d, f"out_{model_name}", "occlusion_mask.npy"), occ)
    return scene


def random_dot_stereogram(width=176, height=120, seed=0):
    """A stereo pair with a known disparity for the matcher's tests: (left, right, true_disparity).  ``left`` / ``right`` are
    [H,W,3] u8 with equal channels (so the matcher's grey value is the channel value), ``true_disparity`` [H,W] f64 is the
    left image's: a disc of radius 0.375 H in the centre bulging from 14 px at its rim to 22 px, over a 5 px background.
    The left image is lightly smoothed noise; the right eye is its z-buffered forward warp (nearest pixel wins), holes
    filled with fresh noise."""
    rng = np.random.default_rng(seed)
    H, W = int(height), int(width)
    yy, xx = np.mgrid[:H, :W]
    r2 = ((xx - W / 2) ** 2 + (yy - H / 2) ** 2) / (0.375 * H) ** 2
    dtrue = np.where(r2 < 1, 14.0 + 8.0 * np.sqrt(np.clip(1 - r2, 0, 1)), 5.0)
    left = rng.integers(0, 256, (H, W)).astype(np.int32)
    left = (left + np.roll(left, 1, 0) + np.roll(left, 1, 1) + np.roll(left, (1, 1), (0, 1))) // 4
    right = rng.integers(0, 256, (H, W)).astype(np.int32)
    shift = np.rint(dtrue).astype(np.int64)
    xr = xx - shift
    order = np.argsort(dtrue, axis=None, kind="stable")          # far to near: the nearest source is written last
    oy, ox = np.unravel_index(order, (H, W))
    ok = (xr[oy, ox] >= 0) & (xr[oy, ox] < W)
    right[oy[ok], xr[oy, ox][ok]] = left[oy[ok], ox[ok]]
    to_rgb = lambda g: np.ascontiguousarray(np.repeat(g.astype(np.uint8)[:, :, None], 3, axis=2))
    return to_rgb(left), to_rgb(right), dtrue


def textured_sphere(P, seed, radius=0.6, sigma=0.02):
    """Gaussians (GaussianModel layout, like ``synth_v1``) of a matchable surface: P opaque isotropic splats of scale
    ``sigma`` with random DC colours on the sphere of ``radius`` around the origin, zero rest SH (the same colour from
    every direction, as stereo assumes)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * radius).astype(np.float32)
    scaling = np.full((P, 3), np.log(sigma), np.float32)
    rotation = np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1))
    o = np.full((P, 1), 0.95)
    opacity = np.log(o / (1 - o)).astype(np.float32)
    f_dc = RGB2SH(rng.uniform(0, 1, size=(P, 1, 3))).astype(np.float32)
    return dict(xyz=xyz, features_dc=f_dc, features_rest=np.zeros((P, 15, 3), np.float32), scaling=scaling,
                rotation=rotation, opacity=opacity)


def surfel_sphere(P, seed, radius=0.6, sigma=0.03, thickness=1e-4):
    """``textured_sphere`` with FLAT discs: P opaque splats of scales (sigma, sigma, thickness) on the sphere of ``radius``,
    each rotated so that its thin axis is the sphere's normal at its centre -- a splat that carries the surface's orientation,
    as a trained one does.  The tangent plane of a disc of radius 3 sigma leaves the sphere by about (3 sigma)^2 / (2 radius)."""
    rng = np.random.default_rng(seed)
    g = textured_sphere(P, seed, radius, sigma)
    n = g["xyz"].astype(np.float64) / radius
    # the shortest rotation that takes +z to n: q = (1 + n_z, -n_y, n_x, 0), normalised (n = -z: a half turn about x)
    q = np.stack([1.0 + n[:, 2], -n[:, 1], n[:, 0], np.zeros(P)], axis=1)
    flip = np.linalg.norm(q, axis=1) < 1e-6
    q[flip] = [0.0, 1.0, 0.0, 0.0]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g["rotation"] = q.astype(np.float32)
    g["scaling"] = np.log(np.tile(np.array([sigma, sigma, thickness]), (P, 1))).astype(np.float32)
    g["features_dc"] = RGB2SH(rng.uniform(0, 1, size=(P, 1, 3))).astype(np.float32)
    return g
