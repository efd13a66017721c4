"""3DGS training end to end on the GPU: initialisation from a point cloud (distCUDA2 on the HIP kNN kernel), render() as the
gradient path of the loop, and train() on a small synthetic scene."""
import math

import numpy as np
import pytest
import torch

import knn_statement

pytestmark = pytest.mark.gpu

ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.fixture(autouse=True)
def device_memory():
    from backends import use_host_memory
    use_host_memory(False)


def test_create_from_pcd():
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.graphics import BasicPointCloud
    from gs2mesh_amd.sh_utils import RGB2SH
    r = np.random.default_rng(0)
    pts = r.normal(0, 1, (500, 3)).astype(np.float32)
    pts[10] = pts[11] = pts[12] = pts[13]                       # a zero distance: the 1e-7 floor
    col = r.uniform(0, 1, (500, 3)).astype(np.float32)
    m = GaussianModel(3, device="cuda")
    m.create_from_pcd(BasicPointCloud(pts, col, np.zeros_like(pts)), 3.85)
    assert m.spatial_lr_scale == 3.85
    for a in ATTRS:
        p = getattr(m, a)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_cuda and p.dtype == torch.float32, a
    st = knn_statement.mean_dist2(pts)
    assert st[10] == 0
    want = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(st).cuda(), 1e-7)))
    got = m._scaling.detach()
    assert got.shape == (500, 3) and torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, math.inf)) - want)
    assert bool(((got[:, 0] - want).abs() <= ulp).all())        # the same torch ops on the same values: within 1 ulp
    assert torch.equal(m._xyz.detach().cpu(), torch.from_numpy(pts))
    assert torch.equal(m._rotation.detach().cpu(), torch.tensor([1.0, 0, 0, 0]).repeat(500, 1))
    assert torch.allclose(m._opacity.detach().cpu(), torch.full((500, 1), math.log(0.1 / 0.9)), rtol=1e-6, atol=0)
    # RGB2SH on the device, as create_from_pcd and the reference apply it (a division by a scalar rounds differently on the host)
    assert torch.equal(m._features_dc.detach(), RGB2SH(torch.from_numpy(col).cuda()).reshape(500, 1, 3))
    assert m._features_rest.shape == (500, 15, 3) and not m._features_rest.detach().any()
    assert m.max_radii2D.shape == (500,) and m.max_radii2D.is_cuda and m.active_sh_degree == 0


def small_model(requires_grad):
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.training import OptimizationParams
    g = synthetic.textured_sphere(400, 3)
    m = GaussianModel(3, device="cuda")
    m.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    if requires_grad:
        m.spatial_lr_scale = 1.0
        m.training_setup(OptimizationParams())
    return m


def camera(i=0, W=96, H=80, focal=165.0):
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.graphics import Camera, focal2fov
    p = synthetic.ring_poses(6)[i]
    return Camera(i, p[:, :3].T, p[:, 3], focal2fov(focal, W), focal2fov(focal, H), W, H)


def test_render_carries_the_gradient_of_the_operator():
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams
    m, cam = small_model(True), camera()
    bg = torch.zeros(3, device="cuda")
    w = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(0)).cuda()
    pkg = render(cam, m, PipelineParams(), bg)
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii"}
    vs = pkg["viewspace_points"]
    assert pkg["render"].requires_grad and vs.requires_grad and vs.shape == m._xyz.shape and not vs.detach().any()
    (pkg["render"] * w).sum().backward()
    assert vs.grad is not None and m._xyz.grad is not None and m._opacity.grad is not None
    # the operator called directly with the same inputs
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda").contiguous()
    rs = GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=dev(cam.world_view_transform),
        projmatrix=dev(cam.full_proj_transform), sh_degree=m.active_sh_degree, campos=dev(cam.camera_center),
        prefiltered=False, debug=False)
    m2d = torch.zeros_like(m._xyz, requires_grad=True)
    img, radii = GaussianRasterizer(rs)(means3D=m.get_xyz, means2D=m2d, shs=m.get_features, opacities=m.get_opacity,
                                        scales=m.get_scaling, rotations=m.get_rotation)
    (img * w).sum().backward()
    assert torch.equal(img.detach(), pkg["render"].detach()) and torch.equal(radii, pkg["radii"])
    assert torch.equal(vs.grad, m2d.grad)
    filled = m2d.grad.abs().sum(dim=1) != 0
    assert torch.equal(vs.grad.abs().sum(dim=1) != 0, filled) and 50 < int(filled.sum()) <= int((radii > 0).sum())
    assert torch.equal(pkg["visibility_filter"], radii > 0)


def test_render_without_gradients_is_todays_path():
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams
    plain, cam = small_model(False), camera(1)
    bg = torch.zeros(3, device="cuda")
    a = render(cam, plain, PipelineParams(), bg)                # plain tensors, gradients enabled: nothing to differentiate
    assert not a["render"].requires_grad and not a["viewspace_points"].requires_grad
    m = small_model(True)
    with torch.no_grad():
        b = render(cam, m, PipelineParams(), bg)
    assert not b["render"].requires_grad and not b["viewspace_points"].requires_grad and b["render"].grad_fn is None
    assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"])
    assert float(a["render"].max()) > 0.2


# ---- train() end to end ---------------------------------------------------------------------------------------------------
# densify_grad_threshold for this scene (300 initial Gaussians, 96 x 80, six views): the reference's default, 2e-4, fires here.
# Measured on MI355X (cloned / split / pruned per event):  iteration 40: 1 / 295 / 0 (P 300 -> 596),  60: 69 / 493 / 0
# (-> 1158),  80: 78 / 196 / 33 (-> 1399); mean loss over the six views 0.210 -> 0.089.  The initial scales (~0.1, from the 3-NN
# distance of 300 points on the sphere) start on the split side of percent_dense * extent = 0.0385; divisions by 1.6 and the
# optimisation bring children to the clone side from the second event on.  (5e-5 and 1e-5 select more at iteration 80:
# 476 / 657 and 515 / 682, P -> 2287 and 2339.)
GRAD_THRESHOLD = 2e-4


def run_training(seed=0):
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.training import OptimizationParams, cameras_extent, synthetic_scene, train
    cameras, images, pcd, _, bg = synthetic_scene("cuda", n_true=1500, n_init=300, n_views=6, width=96, height=80)
    extent = cameras_extent(cameras)
    opt = OptimizationParams(iterations=120, densify_from_iter=20, densification_interval=20, densify_until_iter=100,
                             opacity_reset_interval=60, densify_grad_threshold=GRAD_THRESHOLD)
    torch.manual_seed(seed)
    g = GaussianModel(3, device="cuda")
    g.create_from_pcd(pcd, extent)
    g.training_setup(opt)
    events = []

    def lengths_agree(it, event, gm, counts):
        P = gm._xyz.shape[0]
        for grp in gm.optimizer.param_groups:
            p = grp["params"][0]
            assert p.shape[0] == P and p.requires_grad and p.is_leaf, (it, event, grp["name"])
            st = gm.optimizer.state.get(p)
            assert st is not None and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, (it, event, grp["name"])
        for a, grp in zip(ATTRS, gm.optimizer.param_groups):
            assert getattr(gm, a) is grp["params"][0]
        assert gm.xyz_gradient_accum.shape == (P, 1) and gm.denom.shape == (P, 1) and gm.max_radii2D.shape == (P,)
        events.append((it, event, P, counts))

    def evaluate():
        from gs2mesh_amd.gaussian_renderer import render
        from gs2mesh_amd.training import PipelineParams, loss_fn
        with torch.no_grad():
            return float(torch.stack([loss_fn(render(c, g, PipelineParams(), bg)["render"], im, opt.lambda_dssim)
                                      for c, im in zip(cameras, images)]).mean())

    before = evaluate()
    P0 = g._xyz.shape[0]
    losses = train(g, cameras, images, opt, extent=extent, bg=bg, seed=seed, callback=lengths_agree)
    return dict(g=g, losses=losses, events=events, before=before, after=evaluate(), P0=P0, cameras=cameras, bg=bg)


@pytest.fixture(scope="module")
def trained():
    return run_training()


def test_train_lowers_the_loss_and_densifies(trained):
    t = trained
    for it, event, P, counts in t["events"]:
        print(f"iteration {it:3d} {event:13s} P = {P:5d} {counts if counts else ''}")
    print(f"P {t['P0']} -> {t['g']._xyz.shape[0]}; mean loss over the six views {t['before']:.5f} -> {t['after']:.5f}")
    assert len(t["losses"]) == 120 and all(math.isfinite(x) for x in t["losses"])
    assert t["after"] < t["before"]                                                             # 1
    dens = [e for e in t["events"] if e[1] == "densify"]
    assert [e[0] for e in dens] == [40, 60, 80]
    assert [e[0] for e in t["events"] if e[1] == "reset_opacity"] == [60]
    sizes = [t["P0"]] + [e[2] for e in dens]
    assert any(a != b for a, b in zip(sizes, sizes[1:]))                                        # 2
    assert any(e[3]["cloned"] > 0 for e in dens) and any(e[3]["split"] > 0 for e in dens)       # the threshold's purpose
    for a in ATTRS:                                                                             # 4 (3 is the callback)
        assert bool(torch.isfinite(getattr(t["g"], a).detach()).all()), a


def test_train_is_reproducible_up_to_the_first_densification(trained):
    again = run_training()
    first = min(e[0] for e in trained["events"] if e[1] == "densify")
    assert again["losses"][:first] == trained["losses"][:first]                                 # 5
    assert again["g"]._xyz.shape[0] == trained["g"]._xyz.shape[0]
    assert again["before"] == trained["before"]


def test_trained_model_survives_the_ply_round_trip(trained, tmp_path):
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams
    g = trained["g"]
    path = tmp_path / "point_cloud.ply"
    g.save_ply(str(path))
    fresh = GaussianModel(3, device="cuda")
    fresh.load_ply(str(path))
    assert fresh._xyz.shape == g._xyz.shape and not fresh._xyz.requires_grad
    fresh.active_sh_degree = g.active_sh_degree         # the file does not hold it; 120 iterations never raise it
    cam = trained["cameras"][2]
    with torch.no_grad():
        a = render(cam, g, PipelineParams(), trained["bg"])["render"]
        b = render(cam, fresh, PipelineParams(), trained["bg"])["render"]
    assert torch.equal(a, b) and float(a.max()) > 0.2                                           # 6
