"""Ray depth above the C ABI (no GPU, no HIP library): ``render(..., ray_depth=True)``, ``GaussianRasterizer.depth_maps`` with
``expected_ray`` / ``median_ray`` and ``RenderedDepth(kind="ray_median" / "ray_expected")``, with the CPU emulator build of the
kernels behind the operator module's handle (the fixtures of tests/test_rendered_depth.py)."""
import math

import numpy as np
import pytest
import torch

from rendered_depth_scene import np_of, tsdf_args
from test_rendered_depth import H, OLD_KEYS, VIEWS, W, emu, scene  # noqa: F401  (fixtures)


def rasterizer_of(scene, i):
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cam = scene.camera(i)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous()
    return GaussianRasterizer(GaussianRasterizationSettings(
        H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), scene.background, 1.0, t(cam.world_view_transform),
        t(cam.full_proj_transform), 3, t(cam.camera_center), False, False))


def forward_of(r, pc, **kw):
    args = dict(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), opacities=pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation)
    args.update(kw)
    return r(**args)


def test_render_with_ray_depth_adds_two_detached_maps(emu, scene):
    from gs2mesh_amd.gaussian_renderer import render
    cam, pc, bg = scene.left_view(0)
    with torch.no_grad():
        deep = render(cam, pc, None, bg, return_depth=True)
        ray = render(cam, pc, None, bg, return_depth=True, ray_depth=True)
        plain = render(cam, pc, None, bg, ray_depth=True)
    assert set(plain) == OLD_KEYS, "ray_depth without return_depth adds nothing"
    assert set(deep) == OLD_KEYS | {"depth", "median_depth", "alpha"}
    assert set(ray) == set(deep) | {"ray_depth", "ray_median_depth"}
    for k in deep:
        assert torch.equal(ray[k], deep[k]), f"{k} changes with ray_depth"
    alpha = np_of(ray["alpha"])
    for k in ("ray_depth", "ray_median_depth"):
        assert ray[k].shape == (H, W) and ray[k].dtype == torch.float32 and not ray[k].requires_grad
        assert np.isfinite(np_of(ray[k])).all() and ((np_of(ray[k]) > 0) == (alpha >= (0.5 if "median" in k else 1e-30))).all()
    # the same maps through the handle
    h = emu
    pcx = lambda t: t.detach().to(torch.float32).contiguous()
    m = h.depth_maps_ray(pcx(pc.get_xyz), pcx(pc.get_scaling), pcx(pc.get_rotation),
                         torch.as_tensor(np.asarray(cam.world_view_transform), dtype=torch.float32).contiguous(), W, H,
                         math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    assert torch.equal(m["expected"], ray["ray_depth"]) and torch.equal(m["median"], ray["ray_median_depth"])
    assert torch.equal(m["alpha"], ray["alpha"])
    # isotropic splats: the ray meets a Gaussian where it passes nearest its centre -- a depth near the centre's, not equal to it
    both = alpha >= 0.5
    diff = np.abs(np_of(ray["ray_median_depth"]) - np_of(ray["median_depth"]))[both]
    assert 0 < diff.max() < 0.1


def test_depth_maps_serves_ray_maps_and_replays_its_own_forward(emu, scene):
    pc = scene.gaussians
    ra, rb = rasterizer_of(scene, 0), rasterizer_of(scene, 1)
    with pytest.raises(RuntimeError, match="has not run a forward"):
        ra.depth_maps(want=("median_ray",))
    with torch.no_grad():
        forward_of(ra, pc)
        first = ra.depth_maps(want=("expected", "median_ray", "expected_ray", "alpha"))
        only = ra.depth_maps(want=("median_ray",))
        forward_of(rb, pc)
        calls = emu.state_calls
        again = ra.depth_maps(want=("median_ray", "expected_ray"))
        assert emu.state_calls == calls + 1, "the forward was replayed, once"
        other = rb.depth_maps(want=("median_ray",))
        with pytest.raises(ValueError, match="unknown"):
            ra.depth_maps(want=("normal_ray",))
    assert set(first) == {"expected", "median_ray", "expected_ray", "alpha"} and set(only) == {"median_ray"}
    assert torch.equal(only["median_ray"], first["median_ray"])
    for k in again:
        assert torch.equal(first[k], again[k]), k
    assert not torch.equal(other["median_ray"], first["median_ray"])
    assert not torch.equal(first["expected"], first["expected_ray"])


def test_cov3d_precomp_has_no_ray_depth(emu, scene):
    pc = scene.gaussians
    r = rasterizer_of(scene, 0)
    with torch.no_grad():
        forward_of(r, pc, scales=None, rotations=None, cov3D_precomp=pc.get_covariance(1.0))
        centre = r.depth_maps()
        assert set(centre) == {"expected", "median", "alpha"}
        for want in (("median_ray",), ("expected", "expected_ray")):
            with pytest.raises(ValueError, match="scales and rotations"):
                r.depth_maps(want=want)


@pytest.mark.parametrize("kind", ["ray_median", "ray_expected"])
def test_rendered_depth_hands_over_the_ray_maps(emu, scene, kind):
    from gs2mesh_amd.depth_utils import KINDS, RenderedDepth
    from gs2mesh_amd.gaussian_renderer import render
    assert KINDS[kind] == {"ray_median": "ray_median_depth", "ray_expected": "ray_depth"}[kind]
    assert KINDS["median"] == "median_depth" and KINDS["expected"] == "depth"
    args = tsdf_args()
    rd = RenderedDepth(scene.output_dir_root, scene, args, device="cpu", kind=kind)
    assert rd.model_name == "RENDER"
    calls = emu.state_calls
    rd.run(start=1, keep_on_device=True, write_files=False)
    assert emu.state_calls == calls + (VIEWS - 1), "ONE forward per left camera: the ray call replays nothing"
    for i in (1, 2):
        cam, pc, bg = scene.left_view(i)
        with torch.no_grad():
            ref = render(cam, pc, None, bg, return_depth=True, ray_depth=True)
        fr = rd.frame_source(i)
        assert torch.equal(fr["depth"], ref[KINDS[kind]])
        assert torch.equal(fr["occlusion"].to(bool), ref["alpha"] >= 0.5)
    # the default is what it was
    rd0 = RenderedDepth(scene.output_dir_root, scene, args, device="cpu")
    rd0.run(start=2, keep_on_device=True, write_files=False)
    with torch.no_grad():
        ref = render(*scene.left_view(2)[:2], None, scene.background, return_depth=True)
    assert rd0.kind == "median" and torch.equal(rd0.frame_source(2)["depth"], ref["median_depth"])
    with pytest.raises(ValueError, match="kind"):
        RenderedDepth("base", None, None, kind="ray")
