"""What the gradient through the ray depth is for, on the GPU: a depth prior turns flat Gaussians onto the surface.

The scene is the 60 degree tilted plane of flat discs of tests/test_raster_depth_ray.py with every rotation perturbed by a seeded
10..15 degrees about a seeded axis.  The priors are the TRUE plane's depth, analytic, from three cameras that see the plane under
60, 45 and 30 degrees; the images are renders of the unperturbed discs.  ``train`` runs the same few Adam steps on rotations and
positions (every other learning rate 0) with ``lambda_depth > 0``, once with ``depth_kind="ray"`` and once with ``"centre"``.
The centre depth cannot see a rotation except through alpha; the ray depth IS the plane of each disc.  Asserted: the ray run's
depth loss falls, its mean angle between disc normal and plane normal falls, and that angle falls by more than in the centre run.
No absolute figure is fixed; the measured angles are printed (profiles/raster_depth_ray_backward.txt).

Also here: the operator through autograd -- ``render(..., ray_depth=True, depth_grad=True)["ray_depth"].sum().backward()`` fills
``rotation.grad`` with the values of ``Rasterizer.backward(..., ray_depth=True)``.
"""
import numpy as np
import pytest
import torch

from test_raster_depth_ray import TILT_DEG, quat_mul, quat_rot, tilted_plane_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 30
LAMBDA = 1.0
VIEW_TURNS_DEG = (0.0, 15.0, 30.0)      # the plane is seen under 60, 45 and 30 degrees
P0 = np.array([0.0, 0.0, 3.0])
NORMAL = np.array([np.sin(np.radians(TILT_DEG)), 0.0, np.cos(np.radians(TILT_DEG))])


@pytest.fixture(autouse=True)
def device_memory():
    from backends import use_host_memory
    use_host_memory(False)


def cameras_of(W, H, f):
    """cameras turned about the vertical axis through the plane's centre, which stays at view depth 3 on the optical axis
    -> (cameras, [(R, t)] world -> camera)"""
    from gs2mesh_amd import synthetic
    cams, poses = [], []
    for deg in VIEW_TURNS_DEG:
        a = np.radians(deg)
        R = np.array([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
        t = P0 - R @ P0
        n_view = R @ NORMAL
        assert abs(np.degrees(np.arccos(n_view[2])) - (TILT_DEG - deg)) < 1e-9, "the turn takes the tilt down"
        cams.append(synthetic.stereo_cameras(np.concatenate([R, t[:, None]], axis=1), W, H, f, f, 0.245)[0])
        poses.append((R, t))
    return cams, poses


def plane_depth(cam, R, t, W, H):
    """view-space depth of the true plane at every pixel centre of one camera, [H,W]"""
    n, p = R @ NORMAL, R @ P0 + t
    rx = ((2 * np.arange(W) + 1) / W - 1) * cam.tanfovx
    ry = ((2 * np.arange(H) + 1) / H - 1) * cam.tanfovy
    return (n @ p) / (n[0] * rx[None, :] + n[1] * ry[:, None] + n[2])


def perturbed(q, seed=7):
    """every rotation followed by a turn of 10..15 degrees about a random axis (in the disc's own frame)"""
    rng = np.random.default_rng(seed)
    out = []
    for qi in np.asarray(q, np.float64):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.radians(rng.uniform(10.0, 15.0))
        out.append(quat_mul(qi, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])))
    return np.stack(out).astype(np.float32)


def model_of(a, rotations):
    from gs2mesh_amd.gaussian_model import GaussianModel
    g = GaussianModel(3, device=DEV)
    o = np.asarray(a["opacities"], np.float64).reshape(-1, 1)
    shs = np.asarray(a["shs"], np.float32)
    with np.errstate(divide="ignore"):
        # copies: a model that trains must not share memory with the case it was built from
        g.load_arrays(np.array(a["means3D"]), shs[:, :1].copy(), shs[:, 1:].copy(), np.log(np.asarray(a["scales"], np.float64)),
                      np.array(rotations), np.log(o / (1 - o)))
    return g


def normal_angle_deg(g):
    """mean angle between the discs' normals (the third column of R(q / |q|)) and the plane's"""
    q = torch.nn.functional.normalize(g._rotation.detach()).double().cpu().numpy()
    n = np.stack([quat_rot(qi)[:, 2] for qi in q])
    return float(np.degrees(np.arccos(np.clip(np.abs(n @ NORMAL), 0.0, 1.0))).mean())


@pytest.fixture(scope="module")
def problem():
    from backends import use_host_memory
    use_host_memory(False)
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams
    c, _ = tilted_plane_case()
    W, H = c["W"], c["H"]
    cams, poses = cameras_of(W, H, 165.0)
    truth = model_of(c["arrays"], c["arrays"]["rotations"])
    bg = torch.zeros(3, device=DEV)
    images, priors = [], []
    with torch.no_grad():
        for cam, (R, t) in zip(cams, poses):
            pkg = render(cam, truth, PipelineParams(), bg, return_depth=True)
            images.append(pkg["render"].clone())
            plane = torch.tensor(plane_depth(cam, R, t, W, H), dtype=torch.float32, device=DEV)
            priors.append(torch.where(pkg["alpha"] > 0.5, plane, torch.zeros_like(plane)))
    assert all(float((p > 0).float().mean()) > 0.15 for p in priors)
    return dict(case=c, cams=cams, images=images, priors=priors, bg=bg, start=perturbed(c["arrays"]["rotations"]))


def depth_loss(pb, g, kind):
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams, depth_l1_loss
    with torch.no_grad():
        total = 0.0
        for cam, prior in zip(pb["cams"], pb["priors"]):
            pkg = render(cam, g, PipelineParams(), pb["bg"], return_depth=True, ray_depth=True)
            total += float(depth_l1_loss(pkg["ray_depth" if kind == "ray" else "depth"], pkg["alpha"], prior))
    return total / len(pb["cams"])


def run(pb, kind):
    from gs2mesh_amd.training import OptimizationParams, train
    opt = OptimizationParams(iterations=STEPS, position_lr_max_steps=STEPS, densify_until_iter=0, lambda_depth=LAMBDA, depth_kind=kind,
                             feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0, rotation_lr=0.01, position_lr_init=0.0005,
                             position_lr_final=0.0005)
    g = model_of(pb["case"]["arrays"], pb["start"])
    g.spatial_lr_scale = 1.0
    g.training_setup(opt)
    before = (normal_angle_deg(g), depth_loss(pb, g, "ray"))
    train(g, pb["cams"], pb["images"], opt, extent=1.0, bg=pb["bg"], seed=0, depth_priors=pb["priors"])
    return before, (normal_angle_deg(g), depth_loss(pb, g, "ray"))


def test_depth_kind_is_centre_by_default_and_checked():
    from gs2mesh_amd.training import OptimizationParams, train
    assert OptimizationParams().depth_kind == "centre" and OptimizationParams(depth_kind="ray").depth_kind == "ray"
    with pytest.raises(ValueError, match="depth_kind"):
        train(None, [], None, OptimizationParams(depth_kind="surface"), extent=1.0, bg=None)


def test_ray_depth_prior_turns_the_discs_onto_the_plane(problem):
    (a0, l0), (a_ray, l_ray) = run(problem, "ray")
    (b0, _), (a_centre, l_centre) = run(problem, "centre")
    print(f"[depth training] {STEPS} steps, lambda_depth {LAMBDA}: mean normal angle {a0:.2f} deg -> ray {a_ray:.2f}, centre "
          f"{a_centre:.2f}; ray depth L1 against the plane {l0:.4f} -> ray {l_ray:.4f}, centre {l_centre:.4f}")
    # a turn of 10..15 degrees about a random axis tilts the normal by less: the part of the axis along the normal spins the disc
    assert a0 == b0 and 5.0 <= a0 <= 15.0, "both runs start from the same perturbed discs"
    assert l_ray < l0, "the ray run's depth loss falls"
    assert a_ray < a0, "the ray run turns the discs towards the plane"
    assert a0 - a_ray > a0 - a_centre, "and by more than the centre depth does"


def test_render_carries_the_graph_of_the_ray_maps(problem):
    """autograd through render() == one Rasterizer.backward(ray_depth=True) call with grad_depth = 1"""
    from gs2mesh_amd.diff_gaussian_rasterization import _handle
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import OptimizationParams, PipelineParams
    pb = problem
    g = model_of(pb["case"]["arrays"], pb["start"])
    g.training_setup(OptimizationParams())
    cam = pb["cams"][1]
    pkg = render(cam, g, PipelineParams(), pb["bg"], return_depth=True, ray_depth=True, depth_grad=True)
    assert pkg["ray_depth"].requires_grad and pkg["ray_median_depth"].requires_grad and pkg["alpha"].requires_grad
    assert not pkg["depth"].requires_grad and not pkg["median_depth"].requires_grad
    detached = render(cam, g, PipelineParams(), pb["bg"], return_depth=True, ray_depth=True)
    assert not detached["ray_depth"].requires_grad and torch.equal(detached["ray_depth"], pkg["ray_depth"].detach())
    assert torch.equal(detached["depth"], pkg["depth"])
    rot = g.get_rotation.detach().clone().requires_grad_(True)      # the operator's own input: the normalised quaternion
    scales, xyz = g.get_scaling.detach().contiguous(), g.get_xyz.detach().contiguous()
    pkg["ray_depth"].sum().backward()
    got = g._rotation.grad.clone()
    assert float(got.abs().max()) > 0
    # the same call by hand
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV).contiguous()
    h = _handle(xyz.device)
    W, H = cam.image_width, cam.image_height
    common = (t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center), pb["bg"], W, H, cam.tanfovx, cam.tanfovy)
    kw = dict(shs=g.get_features.detach().contiguous(), scales=scales, rotations=rot.detach().contiguous(), sh_degree=g.active_sh_degree)
    h.forward(xyz, g.get_opacity.detach().reshape(-1).contiguous(), *common, **kw)
    raw = h.backward(None, xyz, *common, grad_depth=torch.ones((H, W), device=DEV), ray_depth=True, **kw)
    q = g._rotation.detach().clone().requires_grad_(True)
    torch.nn.functional.normalize(q).backward(raw["rot"])
    assert torch.allclose(got, q.grad, rtol=0, atol=1e-6 * float(got.abs().max()))
    centre = h.backward(None, xyz, *common, grad_depth=torch.ones((H, W), device=DEV), **kw)
    assert not torch.allclose(centre["rot"], raw["rot"], rtol=0, atol=1e-3 * float(raw["rot"].abs().max()))
