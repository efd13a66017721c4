"""Gradients through the depth and opacity maps at the operator level: ``GaussianRasterizer.forward(return_depth=True)`` (the
autograd Function ``_RasterizeGaussiansDepth``) and ``gaussian_renderer.render(..., return_depth=True, depth_grad=True)``.

Two back-ends: the CPU emulator build of the kernels behind the operator module's handle (CPU tensors, as
tests/test_rendered_depth.py does) and, marked ``gpu``, the product on the device.  Oracle and bar: the fp64 statement of
tests/depth_grad_statement.py and TOL_FACTOR x the fp32 statement's own error (tests/test_raster_depth_backward.py).
"""
import math
import types

import numpy as np
import pytest
import torch

import depth_grad_statement as dgs
from backends import BACKENDS
from test_raster_backward import _operator_inputs, _settings, case, check
from test_raster_depth_backward import oracle_of
from test_raster_parity import scene


@pytest.fixture(params=BACKENDS)
def dev(request, monkeypatch):
    """-> the torch device the operator's tensors live on; on ``emu`` the operator module's per-device handle is one Rasterizer
    on the emulator library"""
    from backends import make
    from gs2mesh_amd import _lib
    from gs2mesh_amd import diff_gaussian_rasterization as dgr
    from gs2mesh_amd.rasterizer import Rasterizer
    old = _lib.MEMORY
    be = make(request.param)
    if request.param == "emu":
        h = Rasterizer(0, lib=be.lib)
        monkeypatch.setattr(dgr, "_handle", lambda device: h)
        yield torch.device("cpu")
    else:
        yield torch.device("cuda:0")
    _lib.MEMORY = old


def _grads_of(inp, name):
    h = lambda t: None if t is None else t.grad.detach().cpu().numpy()
    g = dict(mean2D=h(inp["means2D"]), opacity=h(inp["opacities"]), mean3D=h(inp["means3D"]))
    if name == "precomp":
        g.update(color=h(inp["colors_precomp"]), cov3D=h(inp["cov3D_precomp"]))
    else:
        g.update(sh=h(inp["shs"]), scale=h(inp["scales"]), rot=h(inp["rotations"]))
    assert all(v is not None for v in g.values())
    return g


def _loss(outs, w, dev):
    color, _, expected, median, alpha = outs
    t = lambda a: torch.from_numpy(a).to(dev)
    return (color * t(w["wC"])).sum() + (expected * t(w["wD"])).sum() + (median * t(w["wM"])).sum() + (alpha * t(w["wA"])).sum()


@pytest.mark.parametrize("name", ["small800", "precomp"])
def test_forward_with_return_depth_fills_grad_of_every_input(dev, name):
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizer
    c = case(name)
    sets, g64, e32, _ = oracle_of(name, alone=name == "small800")
    inp = _operator_inputs(c, dev)
    r = GaussianRasterizer(_settings(c, dev))
    plain = r(**{k: (None if v is None else v.detach()) for k, v in inp.items()})
    assert isinstance(plain, tuple) and len(plain) == 2, "(color, radii), as the reference returns"
    detached = r.depth_maps()
    outs = r(**inp, return_depth=True)
    assert len(outs) == 5 and all(o.requires_grad for o in (outs[0],) + outs[2:]) and not outs[1].requires_grad
    assert torch.equal(outs[0], plain[0]) and torch.equal(outs[1], plain[1])
    for o, k in zip(outs[2:], ("expected", "median", "alpha")):
        assert torch.equal(o, detached[k]), k
    assert not any(v.requires_grad for v in r.depth_maps().values()), "depth_maps() stays detached"
    _loss(outs, sets[0], dev).backward()
    g = _grads_of(inp, name)
    check(f"operator depth/{name}", g, {k: g64[0][k] for k in g}, e32[0])
    # without gradients wanted the same five outputs come from the plain forward
    with torch.no_grad():
        outs0 = r(**inp, return_depth=True)
    assert len(outs0) == 5 and not any(o.requires_grad for o in outs0)
    assert all(torch.equal(a, b) for a, b in zip(outs0, outs))


def test_a_loss_on_one_map_alone_reaches_the_inputs(dev):
    """an output the loss does not use arrives as None in the backward and is a NULL map for the kernel"""
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizer
    c = case("small800")
    sets, g64, e32, _ = oracle_of("small800", alone=True)
    inp = _operator_inputs(c, dev)
    outs = GaussianRasterizer(_settings(c, dev))(**inp, return_depth=True)
    (outs[3] * torch.from_numpy(sets[2]["wM"]).to(dev)).sum().backward()
    g = _grads_of(inp, "small800")
    check("operator median alone", g, {k: g64[2][k] for k in g}, e32[2])


def test_a_colour_only_loss_has_the_colour_functions_gradients_bit_for_bit(dev):
    """operator-level twin of test_colour_only_call_is_the_colour_backward_bit_for_bit: with the maps ignored by the loss the
    depth Function's backward is the colour Function's -- one shared body, the colour kernels.  200 Gaussians on a 33 x 17
    image: 3 x 2 tiles, partial in both axes"""
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    W, H, f = 33, 17, 30.0
    g, s, q, o, shs, cam, _ = scene(200, 9, W, H, f, log_s=math.log(0.06))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, t(np.array([0.1, 0.2, 0.3])), 1.0,
                                       t(cam.world_view_transform), t(cam.full_proj_transform), 3, t(cam.camera_center), False, False)
    w = t(np.random.default_rng(4).uniform(-1.0, 1.0, (3, H, W)))

    def grads(**kw):
        inp = dict(means3D=t(g["xyz"]), means2D=torch.zeros((200, 3), device=dev), opacities=t(o.reshape(-1, 1)), shs=t(shs),
                   scales=t(s), rotations=t(q))
        for v in inp.values():
            v.requires_grad_(True)
        outs = GaussianRasterizer(rs)(**inp, **kw)
        (outs[0] * w).sum().backward()
        return outs, {k: v.grad for k, v in inp.items()}

    plain, g_colour = grads()
    with_maps, g_depth = grads(return_depth=True)
    assert len(plain) == 2 and len(with_maps) == 5 and torch.equal(plain[0], with_maps[0])
    assert float((with_maps[4] > 0).float().mean()) > 0.3, "the scene covers the image"
    for k in g_colour:
        assert g_colour[k] is not None and float(g_colour[k].abs().max()) > 0, k
        assert torch.equal(g_colour[k], g_depth[k]), k


def test_backward_after_another_forward_replays_its_own(dev):
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizer
    ca, cb = case("small800"), case("precomp")
    sa, g64a, e32a, _ = oracle_of("small800", alone=True)
    sb, g64b, e32b, _ = oracle_of("precomp")
    ia, ib = _operator_inputs(ca, dev), _operator_inputs(cb, dev)
    outs_a = GaussianRasterizer(_settings(ca, dev))(**ia, return_depth=True)
    outs_b = GaussianRasterizer(_settings(cb, dev))(**ib, return_depth=True)
    _loss(outs_a, sa[0], dev).backward()
    ga = _grads_of(ia, "small800")
    check("stale/small800", ga, {k: g64a[0][k] for k in ga}, e32a[0])
    _loss(outs_b, sb[0], dev).backward()
    gb = _grads_of(ib, "precomp")
    check("stale/precomp", gb, {k: g64b[0][k] for k in gb}, e32b[0])


def _model(c, dev, grad=True):
    """what ``render`` reads of a GaussianModel, on the activated arrays of a case"""
    a = c["arrays"]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev).requires_grad_(grad)
    leaves = dict(means3D=t(a["means3D"]), opacities=t(a["opacities"].reshape(-1, 1)), shs=t(a["shs"]), scales=t(a["scales"]),
                  rotations=t(a["rotations"]))
    pc = types.SimpleNamespace(get_xyz=leaves["means3D"], get_opacity=leaves["opacities"], get_features=leaves["shs"],
                               get_scaling=leaves["scales"], get_rotation=leaves["rotations"], active_sh_degree=c["deg"],
                               max_sh_degree=3)
    return pc, leaves


def test_render_with_depth_grad_carries_the_graph_and_the_default_does_not(dev):
    from gs2mesh_amd.gaussian_renderer import render
    c = case("small800")
    sets, g64, e32, _ = oracle_of("small800", alone=True)
    bg = torch.from_numpy(c["bg"]).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    # default: detached maps, the colour gradients of a render without return_depth
    pc0, l0 = _model(c, dev)
    plain = render(c["cam"], pc0, None, bg)
    (plain["render"] * t(sets[0]["wC"])).sum().backward()
    pc1, l1 = _model(c, dev)
    off = render(c["cam"], pc1, None, bg, return_depth=True)
    assert not any(off[k].requires_grad for k in ("depth", "median_depth", "alpha"))
    (off["render"] * t(sets[0]["wC"])).sum().backward()
    for k in l0:
        assert torch.equal(l0[k].grad, l1[k].grad), k
    assert torch.equal(plain["viewspace_points"].grad, off["viewspace_points"].grad)
    # depth_grad=True: the same values, with the graph; every parameter and viewspace_points receive the depth terms
    pc2, l2 = _model(c, dev)
    on = render(c["cam"], pc2, None, bg, return_depth=True, depth_grad=True)
    for k in ("render", "depth", "median_depth", "alpha"):
        assert torch.equal(on[k], off[k]) and on[k].requires_grad, k
    _loss((on["render"], None, on["depth"], on["median_depth"], on["alpha"]), sets[0], dev).backward()
    h = lambda x: x.grad.detach().cpu().numpy()
    g = dict(mean2D=h(on["viewspace_points"]), opacity=h(l2["opacities"]).reshape(-1), mean3D=h(l2["means3D"]), sh=h(l2["shs"]),
             scale=h(l2["scales"]), rot=h(l2["rotations"]))
    check("render depth_grad", g, {k: g64[0][k] for k in g}, e32[0])
    assert not torch.equal(on["viewspace_points"].grad, plain["viewspace_points"].grad), "the depth term is in viewspace_points"
    # under no_grad, or for a model that does not require grad, depth_grad=True is the plain forward
    with torch.no_grad():
        ng = render(c["cam"], pc2, None, bg, return_depth=True, depth_grad=True)
    pc3, _ = _model(c, dev, grad=False)
    nr = render(c["cam"], pc3, None, bg, return_depth=True, depth_grad=True)
    for o in (ng, nr):
        assert not any(o[k].requires_grad for k in ("render", "depth", "median_depth", "alpha"))
        assert torch.equal(o["depth"], off["depth"])


def _fit(render_fn, raw0, target, dtype, dev, steps):
    """plain gradient descent on the depth-only loss of training.depth_l1_loss -> loss curve"""
    from gs2mesh_amd.training import depth_l1_loss
    p = {k: torch.tensor(v, dtype=dtype, device=dev, requires_grad=True) for k, v in raw0.items()}
    lr = dict(xyz=2e-2, opacity=2e-1, scaling=5e-2, rotation=1e-2)
    curve = []
    for _ in range(steps + 1):
        act = dict(means3D=p["xyz"], opacities=torch.sigmoid(p["opacity"]).reshape(-1), scales=torch.exp(p["scaling"]),
                   rotations=torch.nn.functional.normalize(p["rotation"]))
        depth, alpha = render_fn(act)
        loss = depth_l1_loss(depth, alpha, target)
        curve.append(float(loss.detach()))
        if len(curve) > steps:
            break
        grads = torch.autograd.grad(loss, list(p.values()))
        with torch.no_grad():
            for (k, v), g in zip(p.items(), grads):
                v -= lr[k] * g
    return curve


def test_descent_on_a_depth_only_loss_tracks_the_fp64_statement(dev):
    """the method and bar of test_raster_backward.test_fit_through_the_operator_tracks_the_fp64_statement, on a depth-only
    loss, at a size the CPU statement differentiates in a few seconds: 250 Gaussians, 48 x 40 pixels, 6 steps"""
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    W, H, f, steps = 48, 40, 45.0, 6
    g, s, q, o, shs, cam, _ = scene(250, 5, W, H, f, log_s=math.log(0.06))
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, t(bg), 1.0, t(cam.world_view_transform),
                                       t(cam.full_proj_transform), 3, t(cam.camera_center), False, False)
    shs_t = t(shs)

    def hip_render(act):
        P = act["means3D"].shape[0]
        out = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros((P, 3), device=dev), opacities=act["opacities"],
                                     shs=shs_t, scales=act["scales"], rotations=act["rotations"], return_depth=True)
        return out[2], out[4]

    shs64 = torch.tensor(shs, dtype=torch.float64)

    def statement_render(act):
        p = dict(act, shs=shs64, means2D=torch.zeros((act["means3D"].shape[0], 3), dtype=torch.float64))
        _, expected, _, alpha, _ = dgs.render(p, cam, W, H, bg, 3, 1.0)
        return expected, alpha

    with torch.no_grad():
        target = hip_render(dict(means3D=t(g["xyz"]), opacities=t(o.reshape(-1)), scales=t(s), rotations=t(q)))[0].clone()
    assert float((target > 0).float().mean()) > 0.3
    rng = np.random.default_rng(3)
    raw0 = dict(xyz=g["xyz"] + rng.normal(0, 0.03, g["xyz"].shape), opacity=g["opacity"].reshape(-1) + rng.normal(0, 0.3, o.size),
                scaling=g["scaling"] + rng.normal(0, 0.1, s.shape), rotation=g["rotation"] + rng.normal(0, 0.05, q.shape))
    raw0 = {k: np.asarray(v, np.float32) for k, v in raw0.items()}
    hip = _fit(hip_render, raw0, target, torch.float32, dev, steps)
    ref = _fit(statement_render, raw0, target.double().cpu(), torch.float64, torch.device("cpu"), steps)
    print("depth fit hip      :", " ".join(f"{x:.6f}" for x in hip))
    print("depth fit statement:", " ".join(f"{x:.6f}" for x in ref))
    assert ref[-1] < ref[0]
    assert hip[-1] <= 1.1 * ref[-1], (hip[-1], ref[-1])
