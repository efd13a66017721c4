"""The fused training update on the GPU: ``optim.FusedAdam`` under the optimiser surgery of ``GaussianModel``, its checkpoint
interchange with ``torch.optim.Adam``, and ``train()`` with ``optimizer_type`` "fused" and "sparse_adam" on the scene of
tests/test_training_gpu.py (300 -> ~1400 Gaussians, 96 x 80, 120 iterations)."""
import copy
import math
import os
import re

import numpy as np
import pytest
import torch

import adam_statement as st

pytestmark = pytest.mark.gpu

ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
GRAD_THRESHOLD = 2e-4                   # tests/test_training_gpu.py: the reference's default fires on this scene
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs2mesh_amd.h")


@pytest.fixture(autouse=True)
def device_memory():
    from backends import use_host_memory
    use_host_memory(False)


def header_number(name):
    return float(re.search(rf"#define {name}\s+([0-9.]+)", open(HEADER).read()).group(1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def options(optimizer_type, iterations=120):
    from gs2mesh_amd.training import OptimizationParams
    return OptimizationParams(iterations=iterations, densify_from_iter=20, densification_interval=20, densify_until_iter=100,
                              opacity_reset_interval=60, densify_grad_threshold=GRAD_THRESHOLD, optimizer_type=optimizer_type)


def fresh_model(optimizer_type, seed=0):
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.training import cameras_extent, synthetic_scene
    cameras, images, pcd, _, bg = synthetic_scene("cuda", n_true=1500, n_init=300, n_views=6, width=96, height=80)
    extent = cameras_extent(cameras)
    opt = options(optimizer_type)
    torch.manual_seed(seed)
    g = GaussianModel(3, device="cuda")
    g.create_from_pcd(pcd, extent)
    g.training_setup(opt)
    return g, opt, cameras, images, bg, extent


# ---- the class ----------------------------------------------------------------------------------------------------------
def test_training_setup_builds_the_stated_optimiser():
    from gs2mesh_amd.optim import FusedAdam
    from gs2mesh_amd.training import OptimizationParams
    assert OptimizationParams().optimizer_type == "default"
    assert not issubclass(FusedAdam, torch.optim.Adam) and issubclass(FusedAdam, torch.optim.Optimizer)
    g = fresh_model("default")[0]
    assert type(g.optimizer) is torch.optim.Adam and not isinstance(g.optimizer, FusedAdam)
    for kind in ("fused", "sparse_adam"):
        g = fresh_model(kind)[0]
        assert type(g.optimizer) is FusedAdam
        assert [grp["name"] for grp in g.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
        assert all(grp["eps"] == 1e-15 and grp["betas"] == (0.9, 0.999) for grp in g.optimizer.param_groups)
    with pytest.raises(ValueError, match="optimizer_type"):
        fresh_model("adamw")


# ---- one step against the statement, through the surgery --------------------------------------------------------------------
def snapshot(g):
    """group name -> (p, m, v, step, lr) on the host; zero moments and step 0 before the first step"""
    out = {}
    for grp in g.optimizer.param_groups:
        p = grp["params"][0]
        s = g.optimizer.state.get(p, {})
        host = lambda t: t.detach().cpu().numpy().copy()
        m = host(s["exp_avg"]) if s else np.zeros(p.shape, np.float32)
        v = host(s["exp_avg_sq"]) if s else np.zeros(p.shape, np.float32)
        out[grp["name"]] = (host(p), m, v, int(s["step"]) if s else 0, grp["lr"])
    return out


def step_and_check(g, rng, visible=None):
    """random gradients, one FusedAdam.step, every tensor against the statement bit for bit"""
    before = snapshot(g)
    grads = {}
    for grp in g.optimizer.param_groups:
        p = grp["params"][0]
        grads[grp["name"]] = (rng.normal(0, 1, tuple(p.shape)) * 10.0 ** rng.uniform(-8, 0, tuple(p.shape))).astype(np.float32)
        p.grad = torch.from_numpy(grads[grp["name"]]).cuda()
    g.optimizer.step(visible=None if visible is None else torch.from_numpy(visible).cuda())
    after = snapshot(g)
    for name, (p, m, v, t, lr) in before.items():
        ref = st.adam(p, grads[name], m, v, lr, (0.9, 0.999), 1e-15, t + 1, visible)
        assert after[name][3] == t + 1, name
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), after[name][:3], ref):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {what}")
    g.optimizer.zero_grad(set_to_none=True)
    return after


def test_step_equals_the_statement_before_and_after_the_surgery():
    g = fresh_model("fused")[0]
    rng = np.random.default_rng(0)
    step_and_check(g, rng)
    s0 = step_and_check(g, rng)
    P = g._xyz.shape[0]
    # prune: the moments follow their rows
    drop = np.zeros(P, bool)
    drop[::7] = True
    g.prune_points(torch.from_numpy(drop).cuda())
    s1 = snapshot(g)
    for name in s0:
        for k in range(3):
            np.testing.assert_array_equal(bits(s1[name][k]), bits(s0[name][k][~drop]), err_msg=name)
        assert s1[name][3] == 2
    # append: new rows start at zero, the step count is kept
    n_new = 37
    new = {name: torch.from_numpy(rng.normal(0, 1, (n_new,) + s1[name][0].shape[1:]).astype(np.float32)).cuda() for name in s1}
    g.densification_postfix(new["xyz"], new["f_dc"], new["f_rest"], new["opacity"], new["scaling"], new["rotation"])
    s2 = snapshot(g)
    for name in s1:
        np.testing.assert_array_equal(bits(s2[name][0]), bits(np.concatenate([s1[name][0], new[name].cpu().numpy()])))
        for k in (1, 2):
            np.testing.assert_array_equal(bits(s2[name][k][:-n_new]), bits(s1[name][k]), err_msg=name)
            assert not s2[name][k][-n_new:].any()
        assert s2[name][3] == 2
    step_and_check(g, rng)
    # opacity reset: that tensor's moments start again, its step count does not
    g.reset_opacity()
    s3 = snapshot(g)
    assert not s3["opacity"][1].any() and not s3["opacity"][2].any() and s3["opacity"][3] == 3
    assert s3["xyz"][1].any()
    step_and_check(g, rng)
    # the row-sparse step on the same model: every third row unseen
    vis = np.array([0, 3, 12], np.int32)[np.arange(g._xyz.shape[0]) % 3]
    step_and_check(g, rng, visible=vis)
    for a, grp in zip(ATTRS, g.optimizer.param_groups):
        assert getattr(g, a) is grp["params"][0]


def test_a_parameter_without_gradient_is_skipped():
    g = fresh_model("fused")[0]
    before = snapshot(g)
    g._xyz.grad = torch.ones_like(g._xyz)
    g.optimizer.step()
    after = snapshot(g)
    assert after["xyz"][3] == 1 and not np.array_equal(after["xyz"][0], before["xyz"][0])
    for name in ("f_dc", "f_rest", "opacity", "scaling", "rotation"):
        assert after[name][3] == 0 and np.array_equal(bits(after[name][0]), bits(before[name][0]))


# ---- checkpoints ----------------------------------------------------------------------------------------------------------
def set_grads(g, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for a in ATTRS:
        p = getattr(g, a)
        p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 1e-3


def test_capture_restore_and_the_interchange_with_torch_adam():
    from gs2mesh_amd.optim import FusedAdam
    fused, opt = fresh_model("fused")[:2]
    for k in (1, 2):
        set_grads(fused, k)
        fused.optimizer.step()
    fused.optimizer.zero_grad(set_to_none=True)
    saved = fused.capture()
    twin = fresh_model("fused")[0]
    # a checkpoint as torch.save / torch.load would hand it back: no tensor shared with the live model
    twin.restore(tuple(x.detach().clone() if isinstance(x, torch.Tensor) else copy.deepcopy(x) for x in saved), opt)
    assert type(twin.optimizer) is FusedAdam
    a, b = snapshot(fused), snapshot(twin)
    for name in a:
        assert a[name][3] == b[name][3] == 2
        for k in range(3):
            np.testing.assert_array_equal(bits(a[name][k]), bits(b[name][k]), err_msg=name)
    for m in (fused, twin):
        set_grads(m, 3)
        m.optimizer.step()
    a, b = snapshot(fused), snapshot(twin)
    for name in a:
        np.testing.assert_array_equal(bits(a[name][0]), bits(b[name][0]), err_msg=name)

    # torch.optim.Adam, two steps -> its state dict into FusedAdam -> the third step of each
    plain, opt_plain = fresh_model("default")[:2]
    assert type(plain.optimizer) is torch.optim.Adam
    for k in (1, 2):
        set_grads(plain, k)
        plain.optimizer.step()
    other = fresh_model("fused")[0]
    with torch.no_grad():
        for attr in ATTRS:
            getattr(other, attr).copy_(getattr(plain, attr))
    other.optimizer.load_state_dict(copy.deepcopy(plain.optimizer.state_dict()))
    s = snapshot(other)
    assert all(s[name][3] == 2 and s[name][1].any() for name in s)
    for m in (plain, other):
        set_grads(m, 3)
        m.optimizer.step()
    tol = header_number("GS2M_ADAM_TOL_TORCH_STEP")
    a, b = snapshot(plain), snapshot(other)
    for name in a:
        want = a[name][0].astype(np.float64)
        absw = np.abs(a[name][0])
        u = (np.nextafter(absw, np.float32(np.inf)) - absw).astype(np.float64) + a[name][4] * 2.0 ** -23
        worst = float((np.abs(b[name][0] - want) / u).max())
        print(f"{name}: third step, FusedAdam against torch.optim.Adam: {worst:.3f} u of {tol}")
        assert a[name][3] == b[name][3] == 3 and worst <= tol, name
    # and the other way: FusedAdam's state dict loads into torch.optim.Adam, which steps from it
    back = fresh_model("default")[0]
    back.optimizer.load_state_dict(copy.deepcopy(fused.optimizer.state_dict()))
    set_grads(back, 4)
    back.optimizer.step()
    assert all(int(back.optimizer.state[grp["params"][0]]["step"]) == 4 for grp in back.optimizer.param_groups)
    assert all(bool(torch.isfinite(grp["params"][0]).all()) for grp in back.optimizer.param_groups)
    # a step count stored as an int is accepted
    for grp in other.optimizer.param_groups:
        other.optimizer.state[grp["params"][0]]["step"] = 3
    set_grads(other, 4)
    other.optimizer.step()
    assert all(other.optimizer.state[grp["params"][0]]["step"] == 4 for grp in other.optimizer.param_groups)


# ---- no host wait ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fused", "sparse_adam"])
def test_update_phase_does_not_wait_for_the_device(kind):
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams, loss_fn
    g, opt, cameras, images, bg, _ = fresh_model(kind)
    probe = torch.ones(8, device="cuda")
    for _ in range(2):                                     # the second pass runs on an existing optimiser state
        pkg = render(cameras[0], g, PipelineParams(), bg)
        loss_fn(pkg["render"], images[0], opt.lambda_dssim).backward()
        torch.cuda.synchronize()
        old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                torch.nonzero(probe)
                raises = False
            except RuntimeError:
                raises = True
            if raises:
                with torch.no_grad():
                    g.update_densification_stats(pkg["viewspace_points"], pkg["radii"])
                    g.optimizer.step(visible=pkg["radii"] if kind == "sparse_adam" else None)
                    g.optimizer.zero_grad(set_to_none=True)
        finally:
            torch.cuda.set_sync_debug_mode(old)
        if not raises:
            pytest.skip("this torch build does not raise on torch.nonzero under set_sync_debug_mode('error')")
    assert float(g.denom.max()) == 2.0 and float(g.denom.sum()) > 0                  # the two updates were made
    assert all(int(g.optimizer.state[grp["params"][0]]["step"]) == 2 for grp in g.optimizer.param_groups)


# ---- train() --------------------------------------------------------------------------------------------------------------
def run_training(optimizer_type, iterations=120, seed=0):
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.training import PipelineParams, loss_fn, train
    g, _, cameras, images, bg, extent = fresh_model(optimizer_type, seed)
    opt = options(optimizer_type, iterations)
    events = []

    def lengths_agree(it, event, gm, counts):
        P = gm._xyz.shape[0]
        for grp in gm.optimizer.param_groups:
            p = grp["params"][0]
            assert p.shape[0] == P and p.requires_grad and p.is_leaf, (it, event, grp["name"])
            s = gm.optimizer.state.get(p)
            assert s is not None and s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape, (it, event, grp["name"])
        for a, grp in zip(ATTRS, gm.optimizer.param_groups):
            assert getattr(gm, a) is grp["params"][0]
        assert gm.xyz_gradient_accum.shape == (P, 1) and gm.denom.shape == (P, 1) and gm.max_radii2D.shape == (P,)
        events.append((it, event, P, counts))

    def evaluate():
        with torch.no_grad():
            return float(torch.stack([loss_fn(render(c, g, PipelineParams(), bg)["render"], im, opt.lambda_dssim)
                                      for c, im in zip(cameras, images)]).mean())

    before = evaluate()
    losses = train(g, cameras, images, opt, extent=extent, bg=bg, seed=seed, callback=lengths_agree)
    return dict(g=g, losses=losses, events=events, before=before, after=evaluate())


_RUNS = {}


def trained(kind, iterations=120):
    if (kind, iterations) not in _RUNS:
        _RUNS[kind, iterations] = run_training(kind, iterations)
    return _RUNS[kind, iterations]


@pytest.mark.parametrize("kind", ["fused", "sparse_adam"])
def test_train_lowers_the_loss_and_densifies(kind):
    from gs2mesh_amd.optim import FusedAdam
    t = trained(kind)
    for it, event, P, counts in t["events"]:
        print(f"{kind}: iteration {it:3d} {event:13s} P = {P:5d} {counts if counts else ''}")
    print(f"{kind}: mean loss over the six views {t['before']:.5f} -> {t['after']:.5f}")
    assert type(t["g"].optimizer) is FusedAdam
    assert len(t["losses"]) == 120 and all(math.isfinite(x) for x in t["losses"])
    assert t["after"] < t["before"]
    dens = [e for e in t["events"] if e[1] == "densify"]
    assert [e[0] for e in dens] == [40, 60, 80]
    assert [e[0] for e in t["events"] if e[1] == "reset_opacity"] == [60]
    assert any(e[3]["cloned"] > 0 for e in dens) and any(e[3]["split"] > 0 for e in dens)
    assert t["g"]._xyz.shape[0] > 300
    for a in ATTRS:
        assert bool(torch.isfinite(getattr(t["g"], a).detach()).all()), a


@pytest.mark.parametrize("kind", ["fused", "sparse_adam"])
def test_train_is_reproducible_up_to_the_first_densification(kind):
    again = run_training(kind, iterations=40)            # the first 40 iterations do not depend on the length of the run
    assert again["losses"] == trained(kind)["losses"][:40]


# The two paths differ by the rounding of the Adam step (include/gs2mesh_amd.h: a few ulp of the parameter per step) and by
# nothing else before the first densification: the statistics only feed the densification.  Both runs are deterministic.
# Measured on MI355X: the largest |loss_fused - loss_default| over iterations 1 .. 40 is 5.96e-8 = 2^-24, four ulp of a loss
# (the losses run from 0.2117 to 0.1597); the test allows 8 x that.  The yardstick is the default path.
FUSED_VS_DEFAULT = 2.0 ** -24


def test_fused_follows_the_default_path_up_to_the_first_densification():
    default = trained("default", 40)
    assert type(default["g"].optimizer) is torch.optim.Adam
    fused = trained("fused")
    diff = max(abs(a - b) for a, b in zip(fused["losses"][:40], default["losses"]))
    print(f"largest loss difference, fused against default, iterations 1 .. 40: {diff:.3e} (losses {default['losses'][0]:.4f} "
          f"-> {default['losses'][-1]:.4f})")
    assert len(default["losses"]) == 40
    assert diff <= 8 * FUSED_VS_DEFAULT
