"""The training half of GaussianModel (GS/scene/gaussian_model.py:61-93, 120-175, 210-213, 258-407) on the CPU:
optimiser groups, learning-rate schedule, the optimiser surgery of pruning and densification, the selection rules of
clone / split / prune, the opacity reset, capture / restore, and the scene extent."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from gs2mesh_amd import synthetic
from gs2mesh_amd.gaussian_model import GaussianModel, get_expon_lr_func, inverse_sigmoid
from gs2mesh_amd.graphics import Camera
from gs2mesh_amd.training import OptimizationParams, cameras_extent

ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def make_model(P=40, seed=0, steps=2, scales=None, **opt):
    g = synthetic.synth_v1(P, seed, -3.0)
    if scales is not None:
        g["scaling"] = np.log(np.asarray(scales, np.float32))
    m = GaussianModel(3, device="cpu")
    m.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    m.spatial_lr_scale = 2.0
    o = OptimizationParams(**opt)
    m.training_setup(o)
    r = torch.Generator().manual_seed(seed)
    for _ in range(steps):                              # Adam state exists after a step
        for a in ATTRS:
            p = getattr(m, a)
            p.grad = torch.randn(p.shape, generator=r)
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return m, o


def moments(m):
    return {g["name"]: (m.optimizer.state[g["params"][0]]["exp_avg"], m.optimizer.state[g["params"][0]]["exp_avg_sq"])
            for g in m.optimizer.param_groups}


def params(m):
    return {g["name"]: g["params"][0] for g in m.optimizer.param_groups}


def step_works(m):
    for a in ATTRS:
        p = getattr(m, a)
        p.grad = torch.ones_like(p)
    before = m._xyz.detach().clone()
    m.optimizer.step()
    assert not torch.equal(before, m._xyz.detach())
    for name, p in params(m).items():
        assert m.optimizer.state[p]["exp_avg"].shape == p.shape, name


def test_training_setup_groups_and_parameters():
    m, o = make_model(steps=0)
    groups = m.optimizer.param_groups
    assert [g["name"] for g in groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    want = [o.position_lr_init * 2.0, o.feature_lr, o.feature_lr / 20.0, o.opacity_lr, o.scaling_lr, o.rotation_lr]
    assert [g["lr"] for g in groups] == want
    assert want == [0.00016 * 2.0, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001]
    assert all(g["eps"] == 1e-15 for g in groups) and isinstance(m.optimizer, torch.optim.Adam)
    for g, a in zip(groups, ATTRS):
        p = getattr(m, a)
        assert isinstance(p, nn.Parameter) and p.requires_grad and g["params"][0] is p
    assert m.xyz_gradient_accum.shape == (40, 1) and m.denom.shape == (40, 1) and m.max_radii2D.shape == (40,)
    assert m.percent_dense == 0.01
    assert m.update_learning_rate(0) == pytest.approx(0.00016 * 2.0, rel=1e-12)       # no delay steps: the mult is idle
    lr = m.update_learning_rate(30000)
    assert groups[0]["lr"] == lr and lr == pytest.approx(0.0000016 * 2.0, rel=1e-12)
    m.active_sh_degree = 2
    m.oneupSHdegree()
    m.oneupSHdegree()
    assert m.active_sh_degree == 3


def test_expon_lr_func():
    a, b, n = 1.6e-4, 1.6e-6, 30000
    f = get_expon_lr_func(a, b, max_steps=n)
    assert f(0) == pytest.approx(a, rel=1e-14)
    assert f(n) == pytest.approx(b, rel=1e-14)
    assert f(n // 2) == pytest.approx(math.sqrt(a * b), rel=1e-14)          # log-linear midpoint
    assert f(2 * n) == pytest.approx(b, rel=1e-14) and f(-1) == 0.0
    d = get_expon_lr_func(a, b, lr_delay_steps=100, lr_delay_mult=0.01, max_steps=n)
    assert d(0) == pytest.approx(a * 0.01, rel=1e-14)
    assert d(100) == pytest.approx(f(100), rel=1e-14)
    assert get_expon_lr_func(0.0, 0.0)(5) == 0.0


def test_prune_points_keeps_the_other_rows_everywhere():
    m, _ = make_model()
    m.xyz_gradient_accum = torch.arange(40.0).reshape(40, 1)
    m.denom = torch.arange(40.0).reshape(40, 1) + 100
    m.max_radii2D = torch.arange(40.0) + 200
    old_p = {k: v.detach().clone() for k, v in params(m).items()}
    old_m = {k: (a.clone(), b.clone()) for k, (a, b) in moments(m).items()}
    mask = torch.zeros(40, dtype=torch.bool)
    mask[[0, 3, 17, 39]] = True
    m.prune_points(mask)
    keep = ~mask
    for (name, p), a in zip(params(m).items(), ATTRS):
        assert getattr(m, a) is p and isinstance(p, nn.Parameter) and p.is_leaf and p.requires_grad
        assert torch.equal(p.detach(), old_p[name][keep]), name
        assert torch.equal(moments(m)[name][0], old_m[name][0][keep]), name
        assert torch.equal(moments(m)[name][1], old_m[name][1][keep]), name
    assert torch.equal(m.xyz_gradient_accum[:, 0], torch.arange(40.0)[keep])
    assert torch.equal(m.denom[:, 0], torch.arange(40.0)[keep] + 100)
    assert torch.equal(m.max_radii2D, torch.arange(40.0)[keep] + 200)
    assert len(m.optimizer.state) == 6
    step_works(m)


def test_densification_postfix_appends_rows_with_zero_moments():
    m, _ = make_model()
    m.denom += 3
    old_p = {k: v.detach().clone() for k, v in params(m).items()}
    old_m = {k: (a.clone(), b.clone()) for k, (a, b) in moments(m).items()}
    new = {k: torch.full((5,) + tuple(v.shape[1:]), 0.25) for k, v in old_p.items()}
    m.densification_postfix(new["xyz"], new["f_dc"], new["f_rest"], new["opacity"], new["scaling"], new["rotation"])
    for name, p in params(m).items():
        assert p.shape[0] == 45 and p.is_leaf and p.requires_grad
        assert torch.equal(p.detach()[:40], old_p[name]) and torch.equal(p.detach()[40:], new[name])
        for k in (0, 1):
            assert torch.equal(moments(m)[name][k][:40], old_m[name][k]) and not moments(m)[name][k][40:].any()
    for t, shape in ((m.xyz_gradient_accum, (45, 1)), (m.denom, (45, 1)), (m.max_radii2D, (45,))):
        assert t.shape == shape and not t.any()
    step_works(m)


def two_sided_model():
    """extent 10, percent_dense 0.01: the threshold between clone and split is a largest scale of 0.1"""
    scales = np.full((40, 3), 0.01, np.float32)
    scales[::2, 1] = 0.5                      # even rows are large (one axis suffices)
    scales[6] = 0.09                          # an even row on the small side
    return make_model(scales=scales)


def test_densify_and_clone_selection_and_rows():
    m, _ = two_sided_model()
    grads = torch.zeros(40, 1)
    hot = [1, 2, 5, 6, 9, 10]
    grads[hot] = 0.5
    grads[11] = 0.4999
    grads[13] = 0.5                           # exactly the threshold: selected (>=)
    old = {a: getattr(m, a).detach().clone() for a in ATTRS}
    assert m.densify_and_clone(grads, 0.5, 10.0) == 5
    sel = [1, 5, 6, 9, 13]                    # hot and max scale <= 0.1
    for a in ATTRS:
        t = getattr(m, a).detach()
        assert t.shape[0] == 45 and torch.equal(t[:40], old[a]) and torch.equal(t[40:], old[a][sel]), a
    step_works(m)


def test_densify_and_split_selection_children_and_padding():
    m, _ = two_sided_model()
    grads = torch.zeros(30, 1)                # shorter than the model: rows 30.. count as 0
    grads[[1, 2, 5, 6, 10]] = 0.5
    m._scaling.data[38] = math.log(0.5)       # large, but beyond the padding
    old = {a: getattr(m, a).detach().clone() for a in ATTRS}
    torch.manual_seed(0)
    assert m.densify_and_split(grads, 0.5, 10.0) == 2
    sel = [2, 10]                             # hot and max scale > 0.1
    keep = [i for i in range(40) if i not in sel]
    assert m._xyz.shape[0] == 40 + 2 * 2 - 2
    for a in ATTRS:
        assert torch.equal(getattr(m, a).detach()[:38], old[a][keep]), a      # the parents are gone
    for a in ("_rotation", "_features_dc", "_features_rest", "_opacity"):
        assert torch.equal(getattr(m, a).detach()[38:], old[a][sel].repeat(2, *([1] * (old[a].dim() - 1)))), a
    child = torch.exp(m._scaling.detach()[38:])
    parent = torch.exp(old["_scaling"][sel]).repeat(2, 1)
    torch.testing.assert_close(child, parent / 1.6, rtol=1e-6, atol=0)
    assert (m._xyz.detach()[38:] - old["_xyz"][sel].repeat(2, 1)).abs().max() > 1e-4   # samples of a 0.5-wide Gaussian
    for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D):
        assert t.shape[0] == 42
    step_works(m)


def test_split_children_of_vanishing_parents_sit_at_their_centres():
    scales = np.full((40, 3), 1e-12, np.float32)
    m, _ = make_model(scales=scales)
    m.percent_dense = 0.0                     # every scale is "large"
    grads = torch.zeros(40, 1)
    sel = [3, 4, 21]
    grads[sel] = 1.0
    centres = m._xyz.detach()[sel].clone()
    m.densify_and_split(grads, 0.5, 10.0)
    assert (m._xyz.detach()[37:] - centres.repeat(2, 1)).abs().max() <= 1e-9


def test_densify_and_prune_rules():
    m, _ = two_sided_model()
    m.xyz_gradient_accum = torch.zeros(40, 1)
    m.denom = torch.zeros(40, 1)              # never seen: 0 / 0 = NaN -> 0, selects nothing
    with torch.no_grad():
        m._opacity[:] = inverse_sigmoid(torch.tensor(0.5))
        m._opacity[7] = inverse_sigmoid(torch.tensor(0.0049))
        m._opacity[8] = inverse_sigmoid(torch.tensor(0.0051))
    m.max_radii2D = torch.zeros(40)
    m.max_radii2D[9] = 25.0                   # large on screen
    with torch.no_grad():
        m._scaling[12] = math.log(1.5)        # > 0.1 * extent in the world
    xyz = m._xyz.detach().clone()
    counts = m.densify_and_prune(0.0002, 0.005, 10.0, None)
    assert counts == {"cloned": 0, "split": 0, "pruned": 1}       # NaN ratio selects nothing; only the opacity prune
    assert torch.equal(m._xyz.detach(), xyz[[i for i in range(40) if i != 7]])
    # with a screen-size threshold the world-size prune runs as well (row 12 of the original numbering)
    m.denom = torch.zeros(39, 1)
    counts = m.densify_and_prune(0.0002, 0.005, 10.0, 20)
    assert counts == {"cloned": 0, "split": 0, "pruned": 1}
    assert torch.equal(m._xyz.detach(), xyz[[i for i in range(40) if i not in (7, 12)]])
    # The screen-size prune reads max_radii2D AFTER clone and split went through densification_postfix, which zeroes it
    # (gaussian_model.py:347 before :398), so as in the reference it only sees radii when neither step ran its postfix.
    # With the two steps stubbed out, the rule itself shows: radius > max_screen_size, only when a threshold is given.
    m.densify_and_clone = m.densify_and_split = lambda *a, **k: 0
    m.max_radii2D = torch.zeros(38)
    m.max_radii2D[8] = 25.0                   # row 9 of the original numbering
    assert m.densify_and_prune(0.0002, 0.005, 10.0, None)["pruned"] == 0
    assert m.densify_and_prune(0.0002, 0.005, 10.0, 30)["pruned"] == 0
    assert m.densify_and_prune(0.0002, 0.005, 10.0, 20)["pruned"] == 1
    assert torch.equal(m._xyz.detach(), xyz[[i for i in range(40) if i not in (7, 9, 12)]])
    del m.densify_and_clone, m.densify_and_split
    step_works(m)


def test_add_densification_stats():
    m, _ = make_model()
    vs = torch.zeros(40, 3)
    vs.grad = torch.arange(120.0).reshape(40, 3)
    f = torch.zeros(40, dtype=torch.bool)
    f[[2, 5]] = True
    m.add_densification_stats(vs, f)
    m.add_densification_stats(vs, f)
    want = torch.zeros(40, 1)
    want[[2, 5], 0] = 2 * torch.linalg.norm(vs.grad[[2, 5], :2], dim=1)
    assert torch.equal(m.xyz_gradient_accum, want) and torch.equal(m.denom[:, 0], f.float() * 2)


def test_reset_opacity():
    m, _ = make_model()
    old = torch.sigmoid(m._opacity.detach().clone())
    with torch.no_grad():
        m._opacity[3] = inverse_sigmoid(torch.tensor(0.004))
    old[3] = 0.004
    m.reset_opacity()
    p = params(m)["opacity"]
    assert m._opacity is p and p.is_leaf and p.requires_grad
    torch.testing.assert_close(torch.sigmoid(p.detach()), torch.clamp(old, max=0.01), rtol=1e-5, atol=0)
    assert (old > 0.01).sum() > 20
    a, b = moments(m)["opacity"]
    assert not a.any() and not b.any() and a.shape == p.shape
    assert moments(m)["xyz"][0].any()                     # the other groups keep theirs
    step_works(m)


def test_capture_restore_round_trip():
    m, o = make_model()
    m.active_sh_degree = 2
    m.xyz_gradient_accum += 1.5
    m.denom += 2
    m.max_radii2D += 3
    state = m.capture()
    n = GaussianModel(3, device="cpu")
    n.restore(state, o)
    assert n.active_sh_degree == 2 and n.spatial_lr_scale == 2.0
    for a in ATTRS:
        assert torch.equal(getattr(n, a).detach(), getattr(m, a).detach()), a
    assert torch.equal(n.xyz_gradient_accum, m.xyz_gradient_accum) and torch.equal(n.denom, m.denom)
    assert torch.equal(n.max_radii2D, m.max_radii2D)
    for name in moments(m):
        assert torch.equal(moments(n)[name][0], moments(m)[name][0]) and torch.equal(moments(n)[name][1], moments(m)[name][1])
    step_works(n)


def test_cameras_extent_of_a_ring():
    cams = [Camera(i, p[:, :3].T, p[:, 3], 0.8, 0.7, 64, 48) for i, p in enumerate(synthetic.ring_poses(8, radius=3.5))]
    assert cameras_extent(cams) == pytest.approx(1.1 * 3.5, rel=1e-5)
