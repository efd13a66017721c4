"""The SGM matcher and the drop-in Stereo at size on the MI355X: parity with the numpy statement on a rendered pair, the full
1600 x 1200 / D = 256 shape, and the whole path splat -> render -> depth -> fuse -> mesh with nothing but this repository."""
import os

import numpy as np
import pytest

import sgm_statement
from gs2mesh_amd import synthetic
from gs2mesh_amd.gaussian_model import write_gaussian_ply
from test_pipeline_classes import make_args, write_colmap

pytestmark = pytest.mark.gpu
RADIUS, RING = 0.6, 3.5


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from backends import use_host_memory
    use_host_memory(False)
    return torch


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def rendered_pair(torch, P, sigma, W, H, focal, baseline, seed=7, pose_index=1):
    """[2,H,W,3] u8 on the device: the product's render of a textured sphere from ring pose `pose_index` of 8"""
    from gs2mesh_amd.rasterizer import Rasterizer, camera_from
    g = synthetic.textured_sphere(P, seed, RADIUS, sigma)
    gd = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    gd["raw"] = True
    pose = synthetic.ring_poses(8, RING)[pose_index]
    left, right = synthetic.stereo_cameras(pose, W, H, focal, focal, baseline)
    res = Rasterizer(0).render_views(gd, [camera_from(left), camera_from(right)], want_color=False, want_rgb8=True)
    return res["rgb8"].clone()


def test_medium_size_parity_on_a_rendered_pair(gpu):
    from gs2mesh_amd import stereo_utils
    W, H, focal, D = 640, 480, 1160.0, 128                   # nearest point: 1160 * 0.245 / 2.9 = 98 px
    rgb8 = rendered_pair(gpu, 100_000, 0.0058, W, H, focal, 0.245)
    lr, rl = stereo_utils.sgm_disparity(rgb8[0], rgb8[1], D)
    host = rgb8.cpu().numpy()
    ref_lr, ref_rl, _ = sgm_statement.sgm(host[0], host[1], D)
    np.testing.assert_array_equal(bits(lr), ref_lr.view(np.uint32))
    np.testing.assert_array_equal(bits(rl), ref_rl.view(np.uint32))
    assert 90 < float(lr.max()) <= D - 1


def test_full_size(gpu):
    from gs2mesh_amd import _lib, stereo_utils
    W, H, focal, D = 1600, 1200, 2900.0, 256                 # nearest point: 2900 * 0.245 / 2.9 = 245 px
    rgb8 = rendered_pair(gpu, 300_000, 0.006, W, H, focal, 0.245)
    lib = _lib.get()
    _lib.SCRATCH.clear()
    lr, rl = stereo_utils.sgm_disparity(rgb8[0], rgb8[1], D)
    (scratch,) = _lib.SCRATCH.values()
    assert scratch.numel() * 8 == (lib.gs2m_stereo_sgm_scratch_bytes(W, H, D) + 7) // 8 * 8
    lr2, rl2 = stereo_utils.sgm_disparity(rgb8[0], rgb8[1], D)
    gpu.cuda.synchronize()
    assert gpu.equal(lr, lr2) and gpu.equal(rl, rl2)                                   # determinism
    flipped = gpu.flip(rgb8, dims=[2]).contiguous()
    prot, _ = stereo_utils.sgm_disparity(flipped[1], flipped[0], D, want_rl=False)    # the reference's RL protocol
    np.testing.assert_array_equal(bits(rl), bits(gpu.flip(prot, dims=[1]).contiguous()))
    assert 0.0 <= float(lr.min()) and 235 < float(lr.max()) <= D - 1
    # recorded, not asserted: splats of sigma 0.006 are 6 px wide here and their blended front lies before the sphere
    pose = synthetic.ring_poses(8, RING)[1]
    z = gpu.from_numpy(synthetic.sphere_depth(pose, W, H, focal, focal, W / 2.0, H / 2.0, RADIUS)).cuda()
    inner = gpu.from_numpy(synthetic.sphere_depth(pose, W, H, focal, focal, W / 2.0, H / 2.0, 0.9 * RADIUS) > 0).cuda()
    err = (lr - focal * 0.245 / z)[inner]
    print(f"full size: median error {float(err.median()):.3f} px, within 1 px {float((err.abs() <= 1).float().mean()):.4f}, "
          f"within 2 px {float((err.abs() <= 2).float().mean()):.4f}")


# ---- end to end -------------------------------------------------------------------------------------------------------
E_W, E_H, E_F, E_B, E_D, E_N = 800, 600, 1450.0, 0.245, 128, 8


def e2e_args(**kw):
    a = dict(renderer_baseline_absolute=E_B, stereo_model="SGM", stereo_max_disparity=E_D, stereo_occlusion_threshold=3,
             stereo_warm=False, png_encoder="device", TSDF_use_mask=True, TSDF_voxel=2, TSDF_sdf_trunc=0.04,
             TSDF_cleaning_threshold=1000)
    a.update(kw)
    return make_args(**a)


@pytest.fixture(scope="module")
def chain(gpu, tmp_path_factory):
    """PLY + COLMAP ring on disk -> Renderer -> Stereo("SGM") with files and kept frames"""
    from gs2mesh_amd.renderer_utils import Renderer
    from gs2mesh_amd.stereo_utils import Stereo
    base = tmp_path_factory.mktemp("sgm_e2e")
    g = synthetic.textured_sphere(147_000, 7, RADIUS, 0.0047)
    ply_dir = base / "splatting_output" / "custom" / "scene" / "point_cloud" / "iteration_30000"
    os.makedirs(ply_dir)
    write_gaussian_ply(str(ply_dir / "point_cloud.ply"), g["xyz"], g["features_dc"], g["features_rest"], g["opacity"],
                       g["scaling"], g["rotation"])
    poses = synthetic.ring_poses(E_N, RING)
    write_colmap(str(base / "colmap"), poses, E_W, E_H, E_F, E_F, E_W / 2, E_H / 2)
    args = e2e_args()
    ren = Renderer(str(base), str(base / "colmap"), str(base / "out"), args)
    ren.prepare_renderer()
    stereo = Stereo(str(base), ren, args)
    stereo.run(keep_on_device=True)
    for i, p in enumerate(poses):          # object masks come from outside the stereo stage (run_single.py's DTU branch)
        np.save(os.path.join(ren.render_folder_name(i), "left_mask.npy"),
                synthetic.sphere_depth(p, E_W, E_H, E_F, E_F, E_W / 2.0, E_H / 2.0, RADIUS) > 0)
    return ren, stereo, poses


def test_end_to_end_disparity_on_the_surface(chain):
    """(a) inside the silhouette of a sphere of 0.9 x the radius: >= 99 % visible, >= 99 % of those within 1 px of fx b / z.
    Measured on the MI355X (8 views together): visible 100.00 %, within 1 px 99.95 %, within 0.5 px 89.78 %
    (profiles/stereo_sgm.txt)."""
    ren, stereo, poses = chain
    n = vis = ok1 = ok05 = 0
    for i, p in enumerate(poses):
        out = os.path.join(ren.render_folder_name(i), "out_SGM")
        assert sorted(os.listdir(ren.render_folder_name(i))) == ["left.png", "left_mask.npy", "out_SGM", "right.png"]
        lr, occ = np.load(os.path.join(out, "disparity_LR.npy")), np.load(os.path.join(out, "occlusion_mask.npy"))
        z = synthetic.sphere_depth(p, E_W, E_H, E_F, E_F, E_W / 2.0, E_H / 2.0, RADIUS)
        inner = synthetic.sphere_depth(p, E_W, E_H, E_F, E_F, E_W / 2.0, E_H / 2.0, 0.9 * RADIUS) > 0
        err = np.abs(lr - E_F * E_B / np.where(inner, z, 1.0))
        sel = inner & occ
        n, vis = n + int(inner.sum()), vis + int(sel.sum())
        ok1, ok05 = ok1 + int((err[sel] <= 1).sum()), ok05 + int((err[sel] <= 0.5).sum())
    print(f"e2e disparity: visible {vis / n:.4f}, within 1 px {ok1 / vis:.4f}, within 0.5 px {ok05 / vis:.4f}")
    assert vis / n >= 0.99
    assert ok1 / vis >= 0.99


def test_end_to_end_mesh(chain):
    """(b) the cleaned mesh is non-empty and one component holds >= 90 % of its triangles; (c) the median distance of its
    vertices from the sphere, e = | |v| - 0.6 |, is at most one pixel of disparity error at the ring radius plus one voxel:
    z^2 / (fx b) + voxel = 3.5^2 / (1450 * 0.245) + 2 / 512 = 0.0384.
    Measured on the MI355X: 947 036 triangles in one component, median(e) = 0.00597, 99th percentile 0.00990 (the percentile is recorded, not asserted; profiles/stereo_sgm.txt)."""
    from gs2mesh_amd.tsdf_utils import TSDF
    ren, stereo, _ = chain
    args = e2e_args()
    t = TSDF(ren, stereo, args, "sgm", fuse="batch")
    t.run()
    t.save_mesh()
    t.clean_mesh()
    mesh = t.clean_mesh
    assert os.path.exists(os.path.join(ren.output_dir_root, "sgm_mesh.ply"))
    assert os.path.exists(os.path.join(ren.output_dir_root, "sgm_cleaned_mesh.ply"))
    tri = np.asarray(mesh.triangles)
    assert tri.shape[0] > 10_000
    _, counts, _ = mesh.cluster_connected_triangles()
    assert np.max(counts) >= 0.9 * tri.shape[0]
    e = np.abs(np.linalg.norm(np.asarray(mesh.vertices), axis=1) - RADIUS)
    bound = RING ** 2 / (E_F * E_B) + args.TSDF_voxel / 512
    print(f"e2e mesh: {tri.shape[0]} triangles, largest component {np.max(counts) / tri.shape[0]:.4f}, "
          f"median e {np.median(e):.5f}, p99 e {np.percentile(e, 99):.5f}, bound {bound:.5f}")
    assert np.median(e) <= bound


def test_end_to_end_memory_chain_equals_file_chain(chain):
    """(d) without object masks the in-memory chain and the file chain fuse the same volume bit for bit"""
    from gs2mesh_amd.tsdf_utils import TSDF
    from test_stereo_class import sorted_volume
    ren, stereo, _ = chain
    args = e2e_args(TSDF_use_mask=False)
    files = TSDF(ren, stereo, args, "files", fuse="batch")
    files.run()
    memory = TSDF(ren, stereo, args, "memory", frame_source=stereo.frame_source, fuse="batch")
    memory.run()
    a, b = sorted_volume(files), sorted_volume(memory)
    assert len(a[0]) > 1000
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
