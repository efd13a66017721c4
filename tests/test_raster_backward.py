"""Backward pass of the rasteriser (gs2m_rasterize_backward) against the differentiable fp64 statement of the reference's
forward (tests/raster_statement.py).

Loss: sum(w * image) with fixed seeded weights; w is zeroed on every pixel where the oracle's replay of renderCUDA finds a
decision within 1e-4 of its threshold (the gradient is discontinuous there and fp32 / fp64 may take different sides); at most 1 %
of the pixels may be zeroed.

Tolerance (per gradient tensor, two metrics: max|g - g64| / max|g64| and relative L2): 4 x the error of the SAME statement
evaluated in fp32 on the CPU -- independent of the code under test.  The kernel sums over ~100 contributors in another order
and rebuilds T by division, both O(n 2^-24) effects like the fp32 statement's own.  Measured figures:
profiles/raster_backward.txt.
"""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
import raster_statement as rs
from gs2mesh_amd import _lib, synthetic
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_parity import scene

TOL_FACTOR = 4.0
TENSORS = ("mean2D", "conic", "opacity", "color", "mean3D", "cov3D", "sh", "scale", "rot")


def _camera(W, H, f, az=0.3, ring=3.5):
    pose = synthetic.ring_pose(az, ring)
    pose = np.concatenate([pose[0], pose[1][:, None]], axis=1)
    return synthetic.stereo_cameras(pose, W, H, f, f, 0.245)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(arrays = the operator's inputs (numpy fp32, None where absent), cam, W, H, bg, deg, mod, w[3,H,W], zeroed)"""
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    deg, mod = 3, 1.0
    if name == "ragged3000":
        W, H, f = 200, 136, 180.0
        g, s, q, o, shs, cam, _ = scene(3000, 11, W, H, f)
    elif name in ("small800", "sh0", "scalemod", "precomp"):
        W, H, f = 96, 80, 90.0
        g, s, q, o, shs, cam, _ = scene(800, 5, W, H, f)
        if name == "sh0":
            deg, shs = 0, np.ascontiguousarray(shs[:, :1])
        if name == "scalemod":
            mod = 0.7
    elif name == "trained":
        W, H, f = 136, 104, 120.0
        g = synthetic.trained_like(1500, 23, math.log(0.03), focal=f)
        s, q, o = oracle.activate(g["scaling"], g["rotation"], g["opacity"])
        shs = np.ascontiguousarray(np.concatenate([g["features_dc"], g["features_rest"]], axis=1))
        cam, _ = _camera(W, H, f)
    else:
        raise KeyError(name)
    arrays = dict(means3D=g["xyz"], opacities=o.reshape(-1), shs=shs, colors_precomp=None, scales=s, rotations=q,
                  cov3D_precomp=None)
    geom = oracle.preprocess(g["xyz"], s, q, o, shs, cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                             W, H, cam.tanfovx, cam.tanfovy, sh_degree=deg, scale_modifier=mod)
    if name == "precomp":
        arrays.update(shs=None, scales=None, rotations=None, cov3D_precomp=geom["cov3D"].copy(),
                      colors_precomp=np.random.default_rng(0).uniform(0, 1, (800, 3)).astype(np.float32))
    # pixels with a decision near its threshold: no weight
    pl, ranges = oracle.bin_instances(geom, W, H)
    fb = oracle.render_flip_bounds(W, H, ranges, pl, geom["means2D"], geom["conic_opacity"], 1.0, rel_eps=1e-4)
    near = (fb["n_alpha"].astype(np.int64) + fb["n_T"] + fb["n_power"]) > 0
    w = np.random.default_rng(77).uniform(-1.0, 1.0, (3, H, W)).astype(np.float32)
    w[:, near] = 0.0
    return dict(name=name, arrays=arrays, cam=cam, W=W, H=H, bg=bg, deg=deg, mod=mod, w=w, zeroed=float(near.mean()),
                geom=geom)


def statement_grads(c, dtype):
    p = rs.leaves(c["arrays"], dtype)
    img, aux = rs.render(p, c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    (img * torch.tensor(c["w"], dtype=dtype)).sum().backward()
    z = lambda t, like: np.zeros(like, np.float64) if t is None or t.grad is None else t.grad.detach().numpy().astype(np.float64)
    P = c["arrays"]["means3D"].shape[0]
    ca, cb, cc = aux["t_conic"]
    conic = np.stack([z(ca, P), 0.5 * z(cb, P), np.zeros(P), z(cc, P)], axis=1)   # dL_dconic.y is half the derivative
    g = dict(mean2D=z(p["means2D"], (P, 3)), conic=conic, opacity=z(p["opacities"], P),
             color=z(aux["t_rgb"], (P, 3)), mean3D=z(p["means3D"], (P, 3)), cov3D=z(aux["t_cov3"], (P, 6)),
             sh=None if p["shs"] is None else z(p["shs"], tuple(p["shs"].shape)),
             scale=z(p.get("scales"), (P, 3)), rot=z(p.get("rotations"), (P, 4)))
    return g, img.detach().numpy(), aux


def errors(g, g64):
    """per tensor: (max|g - g64| / max|g64|, relative L2); None where the oracle's tensor is identically zero"""
    out = {}
    for k in TENSORS:
        if g64.get(k) is None:
            continue
        ref = np.asarray(g64[k], np.float64)
        d = np.asarray(g[k], np.float64) - ref
        m, n = np.abs(ref).max(initial=0.0), math.sqrt(float((ref * ref).sum()))
        out[k] = None if m == 0 else (float(np.abs(d).max() / m), float(math.sqrt(float((d * d).sum())) / n))
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """-> (g64, e32 = errors of the fp32 statement, aux of the fp64 run); also asserts that what is differentiated IS the
    reference's function: image within the clean bar of oracle.rasterize_forward, radii / rect equal to oracle.preprocess"""
    c = case(name)
    g64, img64, aux = statement_grads(c, torch.float64)
    a = c["arrays"]
    ref_img, ref_radii, _ = oracle.rasterize_forward(
        a["means3D"], a["opacities"], c["cam"].world_view_transform, c["cam"].full_proj_transform, c["cam"].camera_center,
        c["W"], c["H"], c["cam"].tanfovx, c["cam"].tanfovy, c["bg"], shs=a["shs"], colors_precomp=a["colors_precomp"],
        scales=a["scales"], rotations=a["rotations"], cov3D_precomp=a["cov3D_precomp"], sh_degree=c["deg"],
        scale_modifier=c["mod"])
    keep = c["w"][0] != 0
    assert np.abs(img64 - ref_img)[:, keep].max() <= 2e-4
    np.testing.assert_array_equal(aux["radii"], ref_radii)
    vis = ref_radii > 0
    np.testing.assert_array_equal(aux["rect"][vis], c["geom"]["rect"][vis])
    assert c["zeroed"] <= 0.01, f"{c['zeroed']:.2%} of the pixels sit on a threshold"
    g32, _, _ = statement_grads(c, torch.float32)
    return g64, errors(g32, g64), aux


def hip_grads(be, c, cull=0, rows=1, twice=False):
    a = c["arrays"]
    d = be.dev
    cam = c["cam"]
    r = Rasterizer(0, lib=be.lib)
    r.set_option(_lib.OPT_EXACT_TILE_CULL, cull)
    if rows != 1:
        r.set_option(_lib.OPT_TILE_ROWS, rows)
    dev = {k: d(v) for k, v in a.items() if k not in ("means3D", "opacities")}
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"],
              cam.tanfovx, cam.tanfovy)
    xyz = d(a["means3D"])
    img, radii = r.forward(xyz, d(a["opacities"]), *common, sh_degree=c["deg"], scale_modifier=c["mod"], **dev)
    outs = []
    for _ in range(2 if twice else 1):
        g = r.backward(d(c["w"]), xyz, *common, sh_degree=c["deg"], scale_modifier=c["mod"], want_conic=True, **dev)
        be.sync()
        outs.append({k: (None if v is None else be.host(v).copy()) for k, v in g.items()})
    return (outs if twice else outs[0]), be.host(radii), r


def check(name, g, g64, e32, factor=TOL_FACTOR):
    e = errors(g, g64)
    bad = []
    for k, v in e.items():
        print(f"[{name}] {k:8s} e32 = {e32[k]}  hip = {v}")
        if v is None:
            assert not np.asarray(g[k]).any(), f"{k}: the oracle's gradient is identically zero"
            continue
        for i, metric in enumerate(("max", "l2")):
            if not v[i] <= factor * e32[k][i]:
                bad.append((k, metric, v[i], e32[k][i]))
    assert not bad, f"{name}: beyond {factor} x the fp32 statement's error: {bad}"


CASES = ["ragged3000", "small800", "trained", "scalemod", "precomp", "sh0"]


@pytest.mark.parametrize("name", CASES)
def test_capi_gradients_match_the_statement(backend, name):
    c = case(name)
    g64, e32, aux = oracle_of(name)
    if name == "trained":
        assert aux["capped"] >= 1, "the 0.99 cap must bind in this scene"
    P = c["arrays"]["means3D"].shape[0]
    # NaN-filled outputs: every element must be written
    import gs2mesh_amd.rasterizer as rz
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):
        t = real_empty(like, shape, np_dtype)
        if np_dtype == np.float32:
            t[...] = float("nan")
        return t

    rz._empty = nan_empty
    try:
        g, radii, _ = hip_grads(backend, c)
    finally:
        rz._empty = real_empty
    for k, v in g.items():
        if v is not None:
            assert v.shape[0] == P and np.isfinite(v).all(), f"{k}: not fully written"
    assert not g["mean2D"][:, 2].any()
    inv = radii == 0
    assert inv.any() or name != "ragged3000"
    for k, v in g.items():
        if v is not None:
            assert not v[inv].any(), f"{k}: non-zero gradient for a culled Gaussian"
    check(name, g, g64, e32)


def test_backward_is_bitwise_reproducible(backend):
    (g1, g2), _, _ = hip_grads(backend, case("ragged3000"), twice=True)
    for k in g1:
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k


@pytest.mark.parametrize("cull", [1, 2])
def test_tile_cull_levels_give_the_same_gradients(backend, cull):
    name = "ragged3000"
    g64, e32, _ = oracle_of(name)
    g, _, _ = hip_grads(backend, case(name), cull=cull)
    check(f"{name}/cull{cull}", g, g64, e32)


def test_unsupported_options_are_errors(backend):
    with pytest.raises(RuntimeError, match="TILE_ROWS"):
        hip_grads(backend, case("small800"), rows=2)
    c = case("small800")
    r = Rasterizer(0, lib=backend.lib)
    d = backend.dev
    cam = c["cam"]
    a = c["arrays"]
    with pytest.raises(RuntimeError, match="no state"):
        r.backward(d(c["w"]), d(a["means3D"]), d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center),
                   d(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=d(a["shs"]), scales=d(a["scales"]),
                   rotations=d(a["rotations"]))
    _, _, r = hip_grads(backend, c)
    with pytest.raises(RuntimeError, match="do not match"):
        r.backward(d(c["w"]), d(a["means3D"][:10]), d(cam.world_view_transform), d(cam.full_proj_transform),
                   d(cam.camera_center), d(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=d(a["shs"][:10]),
                   scales=d(a["scales"][:10]), rotations=d(a["rotations"][:10]))
    r.set_option(_lib.OPT_PAIR_BATCH, 2)
    with pytest.raises(RuntimeError, match="PAIR_BATCH"):
        r.backward(d(c["w"]), d(a["means3D"]), d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center),
                   d(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=d(a["shs"]), scales=d(a["scales"]),
                   rotations=d(a["rotations"]))


def test_reserve_ends_the_forward_state(backend):
    """gs2m_raster_reserve may free and reallocate the records, keys and ranges a backward would read: after it the handle has
    no forward state (an error, never a read of freed arenas), and the wrapper's call count has moved so the operator replays"""
    c = case("small800")
    d = backend.dev
    cam, a = c["cam"], c["arrays"]
    _, _, r = hip_grads(backend, c)
    before = r.state_calls
    r.reserve(4 * a["means3D"].shape[0], 2, c["W"], c["H"], 4_000_000)
    assert r.state_calls > before
    with pytest.raises(RuntimeError, match="no state"):
        r.backward(d(c["w"]), d(a["means3D"]), d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center),
                   d(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=d(a["shs"]), scales=d(a["scales"]),
                   rotations=d(a["rotations"]))


def test_scale_gradient_carries_the_scale_modifier(backend):
    """Sigma = R (mod s)^2 R^T: rendering (s, mod) and (mod s, 1) is the same function of Sigma, so dL/ds of the first must be
    mod x dL/ds of the second -- the factor the reference's computeCov3D omits (backward.cu:321-325) and this library keeps"""
    c = case("scalemod")
    assert c["mod"] != 1.0
    g_mod, _, _ = hip_grads(backend, c)
    c1 = dict(c, mod=1.0, arrays=dict(c["arrays"], scales=(np.float32(c["mod"]) * c["arrays"]["scales"]).astype(np.float32)))
    g_one, _, _ = hip_grads(backend, c1)
    scale = np.abs(g_one["scale"]).max()
    assert scale > 0
    np.testing.assert_allclose(g_mod["scale"], c["mod"] * g_one["scale"], rtol=0, atol=1e-4 * c["mod"] * scale)
    np.testing.assert_allclose(g_mod["rot"], g_one["rot"], rtol=0, atol=1e-4 * np.abs(g_one["rot"]).max())


# ---- operator level: GaussianRasterizer + autograd (GPU only) ---------------------------------------------------------

def _settings(c, dev):
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = c["cam"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    return GaussianRasterizationSettings(
        image_height=c["H"], image_width=c["W"], tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=t(c["bg"]),
        scale_modifier=c["mod"], viewmatrix=t(cam.world_view_transform), projmatrix=t(cam.full_proj_transform),
        sh_degree=c["deg"], campos=t(cam.camera_center), prefiltered=False, debug=False)


def _operator_inputs(c, dev, grad=True):
    a = c["arrays"]
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev).requires_grad_(grad)
    P = a["means3D"].shape[0]
    return dict(means3D=t(a["means3D"]), means2D=torch.zeros((P, 3), device=dev, requires_grad=grad), opacities=t(a["opacities"]),
                shs=t(a["shs"]), colors_precomp=t(a["colors_precomp"]), scales=t(a["scales"]), rotations=t(a["rotations"]),
                cov3D_precomp=t(a["cov3D_precomp"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small800", "precomp"])
def test_operator_fills_grad_of_every_input(name):
    from backends import use_host_memory
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizer
    use_host_memory(False)
    c = case(name)
    g64, e32, _ = oracle_of(name)
    dev = torch.device("cuda:0")
    inp = _operator_inputs(c, dev)
    color, radii = GaussianRasterizer(_settings(c, dev))(**inp)
    (color * torch.from_numpy(c["w"]).to(dev)).sum().backward()
    h = lambda t: None if t is None else t.grad.detach().cpu().numpy()
    g = dict(mean2D=h(inp["means2D"]), opacity=h(inp["opacities"]), mean3D=h(inp["means3D"]))
    if name == "precomp":
        g.update(color=h(inp["colors_precomp"]), cov3D=h(inp["cov3D_precomp"]))
    else:
        g.update(sh=h(inp["shs"]), scale=h(inp["scales"]), rot=h(inp["rotations"]))
    assert all(v is not None for v in g.values())
    check(f"operator/{name}", g, {k: g64[k] for k in g}, e32)


@pytest.mark.gpu
def test_operator_backward_after_a_growing_reserve_replays_the_forward():
    from backends import use_host_memory
    from gs2mesh_amd import diff_gaussian_rasterization as dgr
    use_host_memory(False)
    c = case("small800")
    g64, e32, _ = oracle_of("small800")
    dev = torch.device("cuda:0")
    inp = _operator_inputs(c, dev)
    color, _ = dgr.GaussianRasterizer(_settings(c, dev))(**inp)
    dgr._handle(dev).reserve(4 * c["arrays"]["means3D"].shape[0], 2, c["W"], c["H"], 8_000_000)   # reallocates every arena
    (color * torch.from_numpy(c["w"]).to(dev)).sum().backward()
    h = lambda t: t.grad.detach().cpu().numpy()
    g = dict(mean2D=h(inp["means2D"]), opacity=h(inp["opacities"]), mean3D=h(inp["means3D"]), sh=h(inp["shs"]),
             scale=h(inp["scales"]), rot=h(inp["rotations"]))
    check("reserve/small800", g, {k: g64[k] for k in g}, e32)


@pytest.mark.gpu
def test_operator_no_grad_forward_is_the_plain_forward_and_allocates_no_rows():
    from backends import use_host_memory
    from gs2mesh_amd import diff_gaussian_rasterization as dgr
    use_host_memory(False)
    c = case("small800")
    dev = torch.device("cuda:0")
    dgr._HANDLES.clear()
    inp = _operator_inputs(c, dev, grad=True)
    with torch.no_grad():
        color, radii = dgr.GaussianRasterizer(_settings(c, dev))(**inp)
    assert not color.requires_grad
    assert dgr._handle(dev).backward_rows() == (0, 0)
    inp0 = _operator_inputs(c, dev, grad=False)
    color0, radii0 = dgr.GaussianRasterizer(_settings(c, dev))(**inp0)
    assert dgr._handle(dev).backward_rows() == (0, 0)
    a = c["arrays"]
    cam = c["cam"]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    plain, plain_radii = Rasterizer(0).forward(
        t(a["means3D"]), t(a["opacities"]), t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
        t(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=t(a["shs"]), scales=t(a["scales"]), rotations=t(a["rotations"]),
        sh_degree=c["deg"])
    assert torch.equal(color, plain) and torch.equal(color0, plain) and torch.equal(radii, plain_radii)


@pytest.mark.gpu
def test_operator_backward_after_another_forward_replays_its_own():
    """forward A, forward B, backward of A's loss: A's gradients (the handle's state was B's)"""
    from backends import use_host_memory
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizer
    use_host_memory(False)
    ca, cb = case("small800"), case("precomp")
    g64, e32, _ = oracle_of("small800")
    dev = torch.device("cuda:0")
    ia, ib = _operator_inputs(ca, dev), _operator_inputs(cb, dev)
    color_a, _ = GaussianRasterizer(_settings(ca, dev))(**ia)
    color_b, _ = GaussianRasterizer(_settings(cb, dev))(**ib)
    (color_a * torch.from_numpy(ca["w"]).to(dev)).sum().backward()
    h = lambda t: t.grad.detach().cpu().numpy()
    g = dict(mean2D=h(ia["means2D"]), opacity=h(ia["opacities"]), mean3D=h(ia["means3D"]), sh=h(ia["shs"]),
             scale=h(ia["scales"]), rot=h(ia["rotations"]))
    check("stale/small800", g, {k: g64[k] for k in g}, e32)
    (color_b * torch.from_numpy(cb["w"]).to(dev)).sum().backward()
    g64b, e32b, _ = oracle_of("precomp")
    gb = dict(mean2D=h(ib["means2D"]), opacity=h(ib["opacities"]), mean3D=h(ib["means3D"]), color=h(ib["colors_precomp"]),
              cov3D=h(ib["cov3D_precomp"]))
    check("stale/precomp", gb, {k: g64b[k] for k in gb}, e32b)


# ---- fit: 60 Adam steps through the operator vs the same optimisation driven by the fp64 statement ---------------------

def _fit(render_fn, raw0, targets, dtype, dev, steps=60):
    """raw0: dict of pre-activation numpy parameters; render_fn(activated dict, view) -> image[3,H,W].  -> loss curve"""
    p = {k: torch.tensor(v, dtype=dtype, device=dev, requires_grad=True) for k, v in raw0.items()}
    opt = torch.optim.Adam([dict(params=[p["xyz"]], lr=2e-3), dict(params=[p["shs"]], lr=1e-2),
                            dict(params=[p["opacity"]], lr=2e-2), dict(params=[p["scaling"]], lr=5e-3),
                            dict(params=[p["rotation"]], lr=1e-3)])
    curve = []
    for _ in range(steps + 1):
        opt.zero_grad()
        act = dict(means3D=p["xyz"], shs=p["shs"], opacities=torch.sigmoid(p["opacity"]).reshape(-1),
                   scales=torch.exp(p["scaling"]), rotations=torch.nn.functional.normalize(p["rotation"]))
        loss = sum((render_fn(act, v) - targets[v]).abs().mean() for v in range(len(targets)))
        curve.append(float(loss.detach()))
        if len(curve) > steps:
            break
        loss.backward()
        opt.step()
    return curve


@pytest.mark.gpu
def test_fit_through_the_operator_tracks_the_fp64_statement():
    from backends import use_host_memory
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    use_host_memory(False)
    W, H, f = 96, 80, 90.0
    g, s, q, o, shs, left, right = scene(800, 5, W, H, f)
    cams = [left, right]
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    sets = [GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, t(bg), 1.0, t(c.world_view_transform),
                                          t(c.full_proj_transform), 3, t(c.camera_center), False, False) for c in cams]

    def hip_render(act, v):
        P = act["means3D"].shape[0]
        img, _ = GaussianRasterizer(sets[v])(means3D=act["means3D"], means2D=torch.zeros((P, 3), device=dev, requires_grad=True),
                                             opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                             rotations=act["rotations"])
        return img

    def statement_render(act, v):
        p = dict(act)
        p["means2D"] = torch.zeros((act["means3D"].shape[0], 3), dtype=torch.float64)
        return rs.render(p, cams[v], W, H, bg, 3, 1.0)[0]

    with torch.no_grad():
        truth = dict(means3D=t(g["xyz"]), shs=t(shs), opacities=t(o.reshape(-1)), scales=t(s), rotations=t(q))
        targets = [hip_render(truth, v).clone() for v in range(2)]
    rng = np.random.default_rng(3)
    raw0 = dict(xyz=g["xyz"] + rng.normal(0, 0.01, g["xyz"].shape), shs=shs + rng.normal(0, 0.1, shs.shape),
                opacity=g["opacity"].reshape(-1) + rng.normal(0, 0.3, o.size), scaling=g["scaling"] + rng.normal(0, 0.1, s.shape),
                rotation=g["rotation"] + rng.normal(0, 0.05, q.shape))
    raw0 = {k: np.asarray(v, np.float32) for k, v in raw0.items()}
    hip = _fit(hip_render, raw0, targets, torch.float32, dev)
    ref = _fit(statement_render, raw0, [x.double().cpu() for x in targets], torch.float64, torch.device("cpu"))
    print("fit curve hip      :", " ".join(f"{x:.5f}" for x in hip[::5]))
    print("fit curve statement:", " ".join(f"{x:.5f}" for x in ref[::5]))
    assert ref[-1] < ref[0]
    assert hip[-1] <= 1.1 * ref[-1], (hip[-1], ref[-1])
