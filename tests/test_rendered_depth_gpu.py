"""Depth without a matcher on the MI355X, end to end: a splat of ~2 000 Gaussians on a sphere, six ring views at 160 x 120,
``RenderedDepth`` -> ``TSDF`` in memory and through the written ``out_RENDER`` files, and the opacity map against the image."""
import numpy as np
import pytest

from rendered_depth_scene import SPHERE_RADIUS, SplatScene, np_of, tsdf_args
from test_tsdf_batch import assert_same_volume_and_mesh

pytestmark = pytest.mark.gpu
W, H, F, P, VIEWS = 160, 120, 300.0, 2000, 6


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from backends import use_host_memory
    use_host_memory(False)
    return torch


@pytest.fixture(scope="module")
def fused(gpu, tmp_path_factory):
    """-> (scene, RenderedDepth after run, TSDF fused from memory, TSDF fused from the files)"""
    from gs2mesh_amd.depth_utils import RenderedDepth
    from gs2mesh_amd.tsdf_utils import TSDF
    scene = SplatScene(tmp_path_factory.mktemp("render_depth"), VIEWS, W, H, F, P, "cuda:0")
    args = tsdf_args()
    rd = RenderedDepth(scene.output_dir_root, scene, args)
    rd.run(keep_on_device=True, write_files=True)
    rd.close()
    memory = TSDF(scene, rd, args, "memory", frame_source=rd.frame_source, fuse="batch")
    memory.run()
    files = TSDF(scene, rd, args, "files", fuse="batch")
    files.run()
    return scene, rd, memory, files


def test_rendered_depth_fuses_to_a_mesh(fused):
    scene, rd, memory, _ = fused
    assert sorted(rd.frames) == list(range(VIEWS)) and memory.volume.frames_integrated == VIEWS
    fr = rd.frame_source(0)
    assert fr["image"].is_cuda and tuple(fr["image"].shape) == (H, W, 3) and tuple(fr["depth"].shape) == (H, W)
    assert memory.mesh.triangles.shape[0] > 100
    # not judged (no reference value exists): how far the fused vertices are from the sphere the splat's centres lie on
    v = np.asarray(memory.mesh.vertices)
    d = np.abs(np.linalg.norm(v, axis=1) - SPHERE_RADIUS)
    print(f"[rendered depth] mesh of {v.shape[0]} vertices / {memory.mesh.triangles.shape[0]} triangles; |vertex| - radius of the "
          f"splat centres: mean {d.mean():.4f}, median {np.median(d):.4f}, 95 % {np.quantile(d, 0.95):.4f}, max {d.max():.4f} "
          f"(radius {SPHERE_RADIUS}, voxel {1 / 64:.4f})")


def test_files_and_memory_give_the_same_volume(fused):
    _, _, memory, files = fused
    assert files.frame_source is None and files.model_name == "RENDER"
    assert_same_volume_and_mesh(memory, files)


def test_alpha_is_the_weight_of_the_background(gpu, fused):
    """image = C + (1 - alpha) bg, C = the same view on black, within the forward's clean bar (2e-4 per value,
    include/gs2mesh_amd.h at gs2m_render_views) on every pixel without a renderCUDA decision within 1e-4 of its threshold"""
    import oracle
    from gs2mesh_amd.gaussian_renderer import render
    torch = gpu
    scene = fused[0]
    cam, pc, _ = scene.left_view(0)
    bg = torch.tensor([0.9, 0.5, 0.2], device="cuda:0")
    with torch.no_grad():
        out = render(cam, pc, None, bg, return_depth=True)
        black = render(cam, pc, None, torch.zeros(3, device="cuda:0"))["render"]
    g = scene.arrays
    s, q, o = oracle.activate(g["scaling"], g["rotation"], g["opacity"])
    shs = np.ascontiguousarray(np.concatenate([g["features_dc"], g["features_rest"]], axis=1))
    geom = oracle.preprocess(g["xyz"], s, q, o, shs, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, W, H,
                             cam.tanfovx, cam.tanfovy, sh_degree=3)
    pl, ranges = oracle.bin_instances(geom, W, H)
    fb = oracle.render_flip_bounds(W, H, ranges, pl, geom["means2D"], geom["conic_opacity"], 1.0, rel_eps=1e-4)
    near = (fb["n_alpha"].astype(np.int64) + fb["n_T"] + fb["n_power"]) > 0
    assert near.mean() <= 0.05, "the clean bar speaks about pixels without a decision on its threshold: most pixels must be such"
    alpha = np_of(out["alpha"])
    assert 0.05 < (alpha >= 0.5).mean() < 0.95 and alpha.max() <= 1.0 and alpha.min() == 0.0
    want = np_of(black) + (1.0 - alpha)[None] * np_of(bg)[:, None, None]
    err = np.abs(np_of(out["render"]) - want)[:, ~near].max()
    print(f"[rendered depth] |image - (C + (1 - alpha) bg)| max = {err:.3e} on {(~near).mean():.2%} of the pixels")
    assert err <= 2e-4
