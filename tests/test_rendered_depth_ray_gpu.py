"""Ray depth without a matcher on the MI355X, end to end, on the splat of tests/rendered_depth_scene.py at its smallest test size
(1 200 Gaussians, three ring views at 96 x 72): ``RenderedDepth(kind="ray_median")`` hands ``TSDF`` the bits of
``GaussianRasterizer.depth_maps(want=("median_ray",))`` and they fuse to a mesh; the default kind is untouched.  No mesh-quality
assertion: the sphere's splats are isotropic and carry no surface orientation."""
import math

import numpy as np
import pytest

from rendered_depth_scene import SplatScene, tsdf_args

pytestmark = pytest.mark.gpu
W, H, F, P, VIEWS = 96, 72, 180.0, 1200, 3


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from backends import use_host_memory
    use_host_memory(False)
    return torch


@pytest.fixture(scope="module")
def scene(gpu, tmp_path_factory):
    return SplatScene(tmp_path_factory.mktemp("render_depth_ray"), VIEWS, W, H, F, P, "cuda:0")


def operator_maps(torch, scene, i, want, **override):
    """one forward of left camera i through GaussianRasterizer, then its depth_maps(want)"""
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cam, pc, bg = scene.left_view(i)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda:0").contiguous()
    r = GaussianRasterizer(GaussianRasterizationSettings(
        H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0, t(cam.world_view_transform),
        t(cam.full_proj_transform), pc.active_sh_degree, t(cam.camera_center), False, False))
    args = dict(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), opacities=pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation)
    args.update(override)
    with torch.no_grad():
        r(**args)
        return r, r.depth_maps(want=want)


def test_ray_median_frames_are_the_operators_bits_and_fuse(gpu, scene):
    torch = gpu
    from gs2mesh_amd.depth_utils import RenderedDepth
    from gs2mesh_amd.tsdf_utils import TSDF
    args = tsdf_args()
    rd = RenderedDepth(scene.output_dir_root, scene, args, kind="ray_median")
    rd.run(keep_on_device=True, write_files=False)
    assert sorted(rd.frames) == list(range(VIEWS)) and rd._writer is None
    for i in range(VIEWS):
        _, m = operator_maps(torch, scene, i, ("median_ray", "median", "alpha"))
        fr = rd.frame_source(i)
        assert fr["depth"].is_cuda and tuple(fr["depth"].shape) == (H, W)
        assert torch.equal(fr["depth"], m["median_ray"]), f"view {i}"
        assert torch.equal(fr["occlusion"].to(bool), m["alpha"] >= 0.5)
        assert torch.isfinite(m["median_ray"]).all() and torch.equal(m["median_ray"] > 0, m["alpha"] >= 0.5)
        assert not torch.equal(m["median_ray"], m["median"]), "the ray depth is not the centre's"
    tsdf = TSDF(scene, rd, args, "ray", frame_source=rd.frame_source, fuse="batch")
    tsdf.run()
    assert tsdf.volume.frames_integrated == VIEWS and tsdf.mesh.triangles.shape[0] > 100


def test_the_default_kind_gives_the_bits_it_gave(gpu, scene):
    torch = gpu
    from gs2mesh_amd.depth_utils import RenderedDepth
    rd = RenderedDepth(scene.output_dir_root, scene, tsdf_args())
    assert rd.kind == "median"
    rd.run(keep_on_device=True, write_files=False)
    for i in range(VIEWS):
        _, m = operator_maps(torch, scene, i, ("median",))
        assert torch.equal(rd.frame_source(i)["depth"], m["median"]), f"view {i}"
    with pytest.raises(ValueError, match="kind"):
        RenderedDepth(scene.output_dir_root, scene, tsdf_args(), kind="ray")


def test_cov3d_precomp_has_no_ray_depth(gpu, scene):
    torch = gpu
    pc = scene.gaussians
    r, centre = operator_maps(torch, scene, 0, ("median",), scales=None, rotations=None, cov3D_precomp=pc.get_covariance(1.0))
    assert set(centre) == {"median"}
    with pytest.raises(ValueError, match="scales and rotations"):
        r.depth_maps(want=("median_ray",))
