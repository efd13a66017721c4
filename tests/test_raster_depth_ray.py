"""Ray-Gaussian intersection depth maps (gs2m_rasterize_depth_ray, k_ray_records + k_blend_depth<.., true>) against the fp64
statement of their definition (tests/ray_depth_statement.py), on both back-ends.

Exclusions: those of tests/test_raster_depth.py -- pixels where the oracle's replay of renderCUDA finds a decision within 1e-4 of
its threshold (at most 1 %) and pixels where some contributor leaves the transmittance within 1e-4, relative, of 0.5 (at most
0.2 %) -- plus ``grazing``: some contributor with a weight > 0 meets the pixel's ray within about 1.8 degrees of its plane
(den / (sum |w_k|^2 |r|^2) < 1e-3), where num / den loses its digits in fp32.  At most 10 % of the pixels may be grazing; on the
statement: 0 % on small800 and on ragged3000 (seed 11), 5.8 % on trained.

Tolerance on the kept pixels, for ``expected`` and for ``median`` as a VALUE against the fp64 z_j(p) of the statement's median
Gaussian: TOL_FACTOR (4) x the error of the SAME statement evaluated in fp32, plus the floor (8 + 2 sqrt(n)) 2^-24 of
tests/test_raster_depth_edges.py (n = the longest run of contributors), in max|x - x64| / max|x64| and in relative L2.
``alpha`` is bit-equal to gs2m_rasterize_depth's.  Measured figures: profiles/raster_depth_ray.txt (``-s`` prints them).

The quality test is what the maps are for: on a plane of flat discs tilted by 60 degrees the ray maps are the plane, the centre
maps a staircase.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import depth_statement as ds
import ray_depth_statement as rds
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_backward import TOL_FACTOR, case
from test_raster_backward_edges import finish, random_shs
from test_raster_depth import forward, maps_of

CASES = ["small800", "ragged3000", "trained"]
MAPS = ("expected", "median", "alpha")
U = 2.0 ** -24
GRAZING_CAP = 0.10


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """-> (fp64 statement, e32 = {map: errors of the fp32 statement}, keep[H,W], floor); asserts the caps on the exclusions, that
    fp32 and fp64 agree on the median's Gaussian on every kept pixel, and that the scene is not vacuous"""
    c = case(name)
    s64 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float64)
    s32 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float32)
    near = c["w"][0] == 0
    assert c["zeroed"] <= 0.01, f"{name}: {c['zeroed']:.2%} of the pixels sit on a threshold"
    assert s64["near05"].mean() <= 0.002, f"{name}: {s64['near05'].mean():.3%} of the pixels have T within 1e-4 of 0.5"
    assert s64["grazing"].mean() <= GRAZING_CAP, f"{name}: {s64['grazing'].mean():.2%} of the pixels have a grazing contributor"
    keep = ~near & ~s64["near05"] & ~s64["grazing"]
    np.testing.assert_array_equal(s32["median_id"][keep], s64["median_id"][keep])
    np.testing.assert_array_equal(s32["n_contrib"][keep], s64["n_contrib"][keep])
    has = s64["median_id"] >= 0
    assert has.mean() >= 0.10 and not has.all(), f"{name}: {has.mean():.1%} of the pixels have a median"
    e32 = {k: ds.errors(s32[k], s64[k], keep) for k in ("expected", "median")}
    floor = (8 + 2 * np.sqrt(float(s64["n_contrib"].max()))) * U
    for v in s64.values():
        v.setflags(write=False)
    print(f"[{name}] statement: excluded {near.mean():.3%} (threshold) + {s64['near05'].mean():.3%} (T near 0.5) + "
          f"{s64['grazing'].mean():.3%} (grazing); median on {has.mean():.1%} of the pixels; e32 expected = {e32['expected']}, "
          f"median = {e32['median']}; floor = {floor:.3e}")
    return s64, e32, keep, floor


def ray_maps_of(be, r, c, f, want=MAPS):
    """depth_maps_ray of the forward ``f`` (test_raster_depth.forward) into NaN-filled buffers -> dict of host copies; every map
    must come back finite"""
    import gs2mesh_amd.rasterizer as rz
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):
        t = real_empty(like, shape, np_dtype)
        t[...] = float("nan")
        return t

    cam = c["cam"]
    rz._empty = nan_empty
    try:
        m = r.depth_maps_ray(f["xyz"], f["dev"]["scales"], f["dev"]["rotations"], f["common"][0], c["W"], c["H"], cam.tanfovx,
                             cam.tanfovy, scale_modifier=c["mod"], want=want)
        be.sync()
    finally:
        rz._empty = real_empty
    m = {k: be.host(v).copy() for k, v in m.items()}
    for k, v in m.items():
        assert v.shape == (c["H"], c["W"]) and v.dtype == np.float32 and np.isfinite(v).all(), f"{k}: not fully written / not finite"
    return m


def check(name, m, centre_alpha, s64, e32, keep, floor):
    """the contract of the module docstring; prints kernel / e32 per map and metric"""
    bad = []
    for k in ("expected", "median"):
        e = ds.errors(m[k], s64[k], keep)
        print(f"[{name}] {k:8s} e32 = ({e32[k][0]:.3e}, {e32[k][1]:.3e})  kernel = ({e[0]:.3e}, {e[1]:.3e})  floor = {floor:.3e}")
        for i, metric in enumerate(("max", "l2")):
            if not e[i] <= TOL_FACTOR * e32[k][i] + floor:
                bad.append((k, metric, e[i], e32[k][i]))
    assert not bad, f"{name}: beyond {TOL_FACTOR} x the fp32 statement's error + {floor:.2e}: {bad}"
    # no exclusions from here on
    assert m["alpha"].tobytes() == centre_alpha.tobytes(), f"{name}: alpha differs from gs2m_rasterize_depth's"
    assert ((m["median"] > 0) == (m["alpha"] >= 0.5)).all(), f"{name}: depth_median > 0 must hold exactly where alpha >= 0.5"
    # every z_j(p) >= lo >= 0.2f: the median is one of them; the mean of n of them is, but for a rounding per term
    n = float(s64["n_contrib"].max())
    assert (m["median"][m["median"] > 0] >= np.float32(0.2)).all()
    assert (m["expected"][m["expected"] != 0] >= 0.2 * (1 - 2 * (n + 2) * U)).all()
    empty = (s64["n_contrib"] == 0) & keep
    unlisted = np.repeat(np.repeat(s64["tile_len"] == 0, 16, axis=0), 16, axis=1)[:empty.shape[0], :empty.shape[1]]
    for k in MAPS:
        assert not m[k][empty | unlisted].any(), f"{name}: {k} is not exactly 0 on pixels without a contributor"


@pytest.mark.parametrize("name", CASES)
def test_maps_match_the_statement(backend, name):
    c = case(name)
    s64, e32, keep, floor = oracle_of(name)
    r, f = forward(backend, c)
    m = ray_maps_of(backend, r, c, f)
    centre = maps_of(backend, r, c, want=("alpha",))
    check(name, m, centre["alpha"], s64, e32, keep, floor)


def test_two_calls_give_identical_bits(backend):
    c = case("ragged3000")
    r, f = forward(backend, c)
    m1, m2 = ray_maps_of(backend, r, c, f), ray_maps_of(backend, r, c, f)
    for k in MAPS:
        assert m1[k].tobytes() == m2[k].tobytes(), k


def test_cull_levels_give_identical_bits(backend):
    c = case("ragged3000")
    r, f = forward(backend, c, cull=0)
    base = ray_maps_of(backend, r, c, f)
    for cull in (1, 2):
        r, f = forward(backend, c, cull=cull)
        m = ray_maps_of(backend, r, c, f)
        for k in MAPS:
            assert m[k].tobytes() == base[k].tobytes(), f"cull {cull}: {k}"


def test_any_subset_of_outputs(backend):
    c = case("small800")
    r, f = forward(backend, c)
    full = ray_maps_of(backend, r, c, f)
    for n in range(0, 3):
        for want in itertools.combinations(MAPS, n):
            m = ray_maps_of(backend, r, c, f, want=want)
            assert set(m) == set(want)
            for k in want:
                assert m[k].tobytes() == full[k].tobytes(), f"want = {want}: {k}"
    with pytest.raises(ValueError, match="unknown"):
        ray_maps_of(backend, r, c, f, want=("normal",))


def test_the_ray_pass_leaves_the_forward_state_alone(backend):
    """backward and centre maps after depth_maps_ray on the same state == those of a forward without it"""
    c = case("small800")
    d = backend.dev

    def backward(r, f):
        g = r.backward(d(c["w"]), f["xyz"], *f["common"], sh_degree=c["deg"], scale_modifier=c["mod"], want_conic=True, **f["dev"])
        backend.sync()
        return {k: (None if v is None else backend.host(v).copy()) for k, v in g.items()}

    r1, f1 = forward(backend, c)
    calls = r1.state_calls
    before = maps_of(backend, r1, c)
    ray = ray_maps_of(backend, r1, c, f1)
    assert r1.state_calls == calls, "depth_maps_ray does not end the forward state"
    after = maps_of(backend, r1, c)
    for k in MAPS:
        assert before[k].tobytes() == after[k].tobytes(), f"centre {k} before / after the ray call"
    g1 = backward(r1, f1)
    r2, f2 = forward(backend, c)
    g2 = backward(r2, f2)
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None)
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k
    ray_after = ray_maps_of(backend, r1, c, f1)      # and the ray maps after a backward are the ray maps
    for k in MAPS:
        assert ray_after[k].tobytes() == ray[k].tobytes(), k


def test_scale_modifier_is_applied(backend):
    """the statement at scale_modifier 0.7 (test_raster_backward's ``scalemod``): s = scale_modifier * scales in g, sz, lo and hi"""
    c = case("scalemod")
    s64 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float64)
    s32 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float32)
    keep = (c["w"][0] != 0) & ~s64["near05"] & ~s64["grazing"]
    assert keep.mean() >= 0.9
    np.testing.assert_array_equal(s32["median_id"][keep], s64["median_id"][keep])
    e32 = {k: ds.errors(s32[k], s64[k], keep) for k in ("expected", "median")}
    floor = (8 + 2 * np.sqrt(float(s64["n_contrib"].max()))) * U
    r, f = forward(backend, c)
    m = ray_maps_of(backend, r, c, f)
    check("scalemod", m, maps_of(backend, r, c, want=("alpha",))["alpha"], s64, e32, keep, floor)


def test_error_conditions(backend):
    c = case("small800")
    W, H, cam = c["W"], c["H"], c["cam"]
    d = backend.dev
    a = c["arrays"]
    xyz, s, q, vm = d(a["means3D"]), d(a["scales"]), d(a["rotations"]), d(cam.world_view_transform)
    call = lambda r, xyz=xyz, s=s, q=q, W=W, H=H: r.depth_maps_ray(xyz, s, q, vm, W, H, cam.tanfovx, cam.tanfovy)
    r = Rasterizer(0, lib=backend.lib)
    with pytest.raises(RuntimeError, match="no state"):
        call(r)
    with pytest.raises(RuntimeError, match="TILE_ROWS"):
        r2, _ = forward(backend, c, rows=2)
        call(r2)
    r, _ = forward(backend, c)
    with pytest.raises(RuntimeError, match="do not match"):
        call(r, W=W + 1)
    with pytest.raises(RuntimeError, match="do not match"):
        call(r, H=H - 1)
    with pytest.raises(RuntimeError, match="P 799 .* do not match"):
        call(r, xyz=d(a["means3D"][:-1]), s=d(a["scales"][:-1]), q=d(a["rotations"][:-1]))
    with pytest.raises(ValueError, match="scales and rotations"):
        call(r, s=None)
    # the C entry itself: NULL scales / rotations
    out = d(np.zeros((H, W), np.float32))
    ptr, st = _lib._ptr, _lib._stream_of(out, None)
    for s_, q_ in ((None, q), (s, None)):
        rc = backend.lib.gs2m_rasterize_depth_ray(r._h, xyz.shape[0], ptr(xyz), ptr(s_), 1.0, ptr(q_), ptr(vm), cam.tanfovx, cam.tanfovy,
                                                  W, H, ptr(out), None, None, st)
        assert rc == 1 and b"scales / rotations" in backend.lib.gs2m_last_error()
    rc = backend.lib.gs2m_rasterize_depth_ray(r._h, xyz.shape[0], ptr(xyz), ptr(s), 1.0, ptr(q), ptr(vm), cam.tanfovx, cam.tanfovy, W, H,
                                              None, None, None, st)
    assert rc == 0, "all outputs NULL does nothing"
    r.reserve(4 * a["means3D"].shape[0], 2, W, H, 4_000_000)      # may reallocate what the pass reads
    with pytest.raises(RuntimeError, match="no state"):
        call(r)
    r, _ = forward(backend, c)
    r.set_option(_lib.OPT_PAIR_BATCH, 2)
    with pytest.raises(RuntimeError, match="PAIR_BATCH"):
        call(r)
    # a forward that overflowed its arena (far too small on purpose); its status has reached the host after a sync
    r = Rasterizer(0, lib=backend.lib)
    r.reserve(a["means3D"].shape[0], 1, W, H, 64)
    r, _ = forward(backend, c, r=r, sync=False)
    backend.sync()
    with pytest.raises(RuntimeError, match="overflowed"):
        call(r)


def test_render_views_ends_the_forward_state(backend):
    from gs2mesh_amd.rasterizer import camera_from
    from test_raster_parity import scene
    W, H, f = 96, 80, 90.0
    g, s, q, o, shs, left, right = scene(800, 5, W, H, f)
    c = case("small800")
    r, fw = forward(backend, c)
    d = backend.dev
    gauss = dict(xyz=d(g["xyz"]), scaling=d(g["scaling"]), rotation=d(g["rotation"]), opacity=d(g["opacity"]),
                 features_dc=d(g["features_dc"]), features_rest=d(g["features_rest"]), raw=True, sh_degree=3)
    r.render_views(gauss, [camera_from(left)], bg=(0.1, 0.2, 0.3))
    with pytest.raises(RuntimeError, match="no state"):
        r.depth_maps_ray(fw["xyz"], fw["dev"]["scales"], fw["dev"]["rotations"], fw["common"][0], W, H, c["cam"].tanfovx,
                         c["cam"].tanfovy)


def test_no_gaussians_gives_zero_maps(backend):
    c = case("small800")
    empty = dict(c, arrays={k: (None if v is None else v[:0]) for k, v in c["arrays"].items()})
    r, f = forward(backend, empty)
    like = backend.dev(np.zeros(1, np.float32))
    z3, z4 = backend.dev(np.zeros((0, 3), np.float32)), backend.dev(np.zeros((0, 4), np.float32))
    m = r.depth_maps_ray(z3, z3, z4, f["common"][0], c["W"], c["H"], c["cam"].tanfovx, c["cam"].tanfovy, like=like)
    backend.sync()
    for k in MAPS:
        assert not backend.host(m[k]).any(), k


# ---- a scene stated in VIEW space, seen by a camera with a generic pose ---------------------------------------------------------
def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def quat_rot(q):
    """computeCov3D's R(q), q = (r, x, y, z)"""
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def posed_case(name, xyz_view, s, q_view, o, shs, W, H, f, seed):
    """the case dict of ``finish`` (without the weights) for Gaussians given in view space -- centres ``xyz_view``, rotations
    ``q_view`` -- under a camera of a random rotation R_c and translation t (default_rng(seed)): world centres
    R_c^T (x - t), world rotations conj(q_c) q.  The view matrix has no zero and no one in it."""
    import oracle
    from gs2mesh_amd import synthetic
    rng = np.random.default_rng(seed)
    qc = rng.normal(size=4)
    qc /= np.linalg.norm(qc)
    Rc, t = quat_rot(qc), rng.uniform(-1.0, 1.0, 3)
    xyz = ((np.asarray(xyz_view, np.float64) - t) @ Rc).astype(np.float32)
    q = np.stack([quat_mul(qc * np.array([1.0, -1.0, -1.0, -1.0]), qv) for qv in np.asarray(q_view, np.float64)]).astype(np.float32)
    cam = synthetic.stereo_cameras(np.concatenate([Rc, t[:, None]], axis=1), W, H, f, f, 0.245)[0]
    s, shs = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(shs, np.float32)
    o = np.ascontiguousarray(o, np.float32).reshape(-1)
    arrays = dict(means3D=xyz, opacities=o, shs=shs, colors_precomp=None, scales=s, rotations=q, cov3D_precomp=None)
    with np.errstate(all="ignore"):
        geom = oracle.preprocess(xyz, s, q, o, shs, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, W, H,
                                 cam.tanfovx, cam.tanfovy, sh_degree=3)
    return dict(name=name, arrays=arrays, cam=cam, W=W, H=H, bg=np.array([0.1, 0.2, 0.3], np.float32), deg=3, mod=1.0, geom=geom)


# ---- what the maps are for ----------------------------------------------------------------------------------------------------
TILT_DEG, THICKNESS = 60.0, 1e-4


@functools.lru_cache(maxsize=None)
def tilted_plane_case(posed=False):
    """96 x 80, focal 165, identity camera; 24 x 24 discs of scales (0.04, 0.04, 1e-4) and opacity 0.9 on a grid of spacing 0.05,
    jittered by +-0.3 spacings (default_rng(0)), in the plane through (0, 0, 3) tilted by 60 degrees about y
    -> (case, analytic plane depth [H,W]).  ``posed``: the same view-space scene under a camera with a generic pose
    (``posed_case``): M = W R(q) with a full W, where a transposed W would tilt the plane the wrong way."""
    W, H, f = 96, 80, 165.0
    rng = np.random.default_rng(0)
    n, spacing = 24, 0.05
    i, j = np.meshgrid(np.arange(n) - 0.5 * (n - 1), np.arange(n) - 0.5 * (n - 1), indexing="ij")
    ab = (np.stack([i.reshape(-1), j.reshape(-1)], axis=1) + rng.uniform(-0.3, 0.3, (n * n, 2))) * spacing
    th = np.radians(TILT_DEG)
    e1, e2, normal = np.array([np.cos(th), 0.0, -np.sin(th)]), np.array([0.0, 1.0, 0.0]), np.array([np.sin(th), 0.0, np.cos(th)])
    p0 = np.array([0.0, 0.0, 3.0])
    xyz = p0 + ab[:, :1] * e1 + ab[:, 1:] * e2
    q = np.tile(np.array([np.cos(0.5 * th), 0.0, np.sin(0.5 * th), 0.0]), (n * n, 1))      # R_y(60 deg): local z -> the normal
    s = np.tile(np.array([0.04, 0.04, THICKNESS]), (n * n, 1))
    if posed:
        c = posed_case("tilted_plane_posed", xyz, s, q, np.full(n * n, 0.9), random_shs(rng, n * n), W, H, f, seed=1)
    else:
        c = finish("tilted_plane", xyz, s, q, np.full(n * n, 0.9), random_shs(rng, n * n), W, H, f)
    cam = c["cam"]
    rx = ((2 * np.arange(W) + 1) / W - 1) * cam.tanfovx
    ry = ((2 * np.arange(H) + 1) / H - 1) * cam.tanfovy
    plane = (normal @ p0) / (normal[0] * rx[None, :] + normal[1] * ry[:, None] + normal[2])
    return c, plane


@pytest.mark.parametrize("posed", [False, True], ids=["identity", "posed"])
def test_tilted_plane_of_discs_is_the_plane(backend, posed):
    """the ray maps are at least 10 x nearer the analytic plane depth than the centre maps (the statement's ratio: above 1000;
    the 1/10 only has to separate "intersection" from "centre"), under the identity camera and under a generic pose"""
    c, plane = tilted_plane_case(posed)
    if posed:
        vm = np.asarray(c["cam"].world_view_transform, np.float64).reshape(4, 4)
        assert np.abs(vm[:3, :3]).min() > 0.05 and np.abs(vm[:3, :3]).max() < 0.99, "a full view rotation"
    r, f = forward(backend, c)
    centre = maps_of(backend, r, c)
    ray = ray_maps_of(backend, r, c, f)
    solid = ray["alpha"] > 0.9
    assert solid.sum() >= 2000, f"only {solid.sum()} pixels with alpha > 0.9"
    err = lambda m: float(np.abs(m[solid].astype(np.float64) - plane[solid]).mean())
    for k in ("expected", "median"):
        e_ray, e_centre = err(ray[k]), err(centre[k])
        print(f"[tilted plane{' posed' if posed else ''}] {k}: mean |map - plane| centre = {e_centre:.4e}, ray = {e_ray:.4e}, on {solid.sum()} pixels")
        assert e_centre > 0.02, f"{k}: the centre map is no staircase ({e_centre:.3e}): the scene does not test anything"
        assert e_ray <= 0.1 * e_centre, f"{k}: ray {e_ray:.3e} vs centre {e_centre:.3e}"
