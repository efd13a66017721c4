"""Gradients through the ray maps (gs2m_rasterize_backward_depth_ray) at their edges, on both back-ends: the degenerate Gaussians
of the definition (a fronto-parallel disc, an isotropic Gaussian, rank <= 1, all scales 0), every branch of the clamp (hi, lo, the
0.2 floor), lists whose ray records cross the 64-instance staging batches, images below a tile and one pixel over, an id beyond
65536, a listed Gaussian with an infinite scale, and the error paths.  The scenes are built with the blocks of
tests/test_raster_backward_edges.py (identity camera: world = view space), most of them the scenes of
tests/test_raster_depth_ray_edges.py.

Every case asserts its purpose on the fp64 statement (tests/ray_depth_grad_statement.py) first; a statement result is computed
once per case, shared between the back-ends and never modified.

Loss: sum(wC image + wD expected_ray + wM median_ray + wA alpha), seeded weights, zero on threshold pixels, wM also where a T sits
at 0.5.  The two ray exclusions of tests/test_raster_depth_ray_backward.py are applied where they bear on the result: a pixel is
dropped for ``grazing`` or ``near a clamp`` only if the contributor in question takes, or in fp32 may take, its depth from the
quotient.  A clamp that binds away from its threshold gives lo or hi whatever digits t lost, and the fallback's t is z_c itself
(a rank <= 1 Gaussian with sz = 0 has t = lo = hi = z_c on every pixel: all three branches send h to dL/dz_c and the square
root's guard removes the rest).  Without this the clamp cases and the rank <= 1 cases would test nothing.

Bar, as in tests/test_raster_backward_edges.py: per tensor (the check of test_raster_backward) and per Gaussian,
e_i = max_j |g[i,j] - g64[i,j]| / max(n_i, PHI S), at most TOL_FACTOR = 4 x the same metric of the SAME statement in fp32.  An
entry whose sum is ill-conditioned is judged, that entry alone, by the worst of several fp32 evaluations of the statement
(``judge``, as in tests/test_raster_depth_backward_edges.py).
"""
import functools

import numpy as np
import pytest
import torch

import depth_grad_statement as dgs
import ray_depth_grad_statement as rdgs
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_backward import TOL_FACTOR, case as big_case, errors
from test_raster_backward_edges import E32_CEILING, ORDERS, finish, per_gaussian, random_shs, scan_scenes, size_case
from test_raster_depth_ray_backward import hip_grads
from test_raster_depth_ray_edges import (IDENT, fronto_case, infinite_scale_case, isotropic_case, rank1_case, stack_case)

_ORACLES, _ORDERS = {}, {}


def oracle_of(key, build, terms=("wC", "wD", "wM", "wA"), seed=99):
    """-> (case, weights, g64, e32 per tensor, pg32 per Gaussian, aux of the fp64 run)"""
    if key in _ORACLES:
        return _ORACLES[key]
    c = build()
    near = c["w"][0] == 0
    rng = np.random.default_rng(seed)
    base = {k: rng.uniform(-1.0, 1.0, (c["H"], c["W"])).astype(np.float32) for k in ("wD", "wM", "wA")}
    base["wC"] = c["w"]
    base = {k: v for k, v in base.items() if k in terms}
    kept = {}

    def sets(aux):
        off = near | aux["grazing_quotient"] | aux["near_clamp_quotient"]
        w = {k: np.where(off[None] if v.ndim == 3 else off, np.float32(0), v) for k, v in base.items()}
        if "wM" in w:
            w["wM"] = np.where(aux["near05"], np.float32(0), w["wM"])
        kept["w"], kept["off"] = w, float((off | aux["near05"]).mean())
        return [w]

    args = (c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    (g64,), _, aux = rdgs.grads(*args, sets, torch.float64)
    (g32,), _, aux32 = rdgs.grads(*args, [kept["w"]], torch.float32)
    np.testing.assert_array_equal(aux32["radii"], aux["radii"])
    print(f"[{key}] {kept['off']:.2%} of the pixels carry no weight (threshold, T near 0.5, grazing or near a clamp at a quotient)")
    _ORACLES[key] = (c, kept["w"], g64, errors(g32, g64), per_gaussian(g32, g64), aux)
    return _ORACLES[key]


def orders(key, back):
    """-> [(per-tensor errors, per-Gaussian errors)] of ORDERS more fp32 evaluations of the statement, a seeded pixel order
    each; ``back``: with the transmittance multiplied up from the back of the list (the order of the backward pass)"""
    if (key, back) not in _ORDERS:
        c, w, g64, _, _, aux64 = _ORACLES[key]
        args = (c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
        out = []
        for seed in range(1, ORDERS + 1):
            (g32,), _, aux = rdgs.grads(*args, [w], torch.float32, pixel_order_seed=seed, transmittance_from_back=back)
            np.testing.assert_array_equal(aux["radii"], aux64["radii"])
            out.append((errors(g32, g64), per_gaussian(g32, g64)))
        _ORDERS[key, back] = out
    return _ORDERS[key, back]


def judge(name, g):
    """test_raster_depth_backward_edges.judge on this file's statement: the bound is TOL_FACTOR x the row-by-row fp32 statement,
    per tensor and per Gaussian.  Where the kernels exceed it, THAT entry alone is judged by the worst of ORDERS more fp32
    evaluations of the statement in other pixel orders and, if that is not enough, with T built from the back of the list -- the
    statement alone decides that the entry's sum is ill-conditioned.  The factor stays, no yardstick may exceed E32_CEILING, and
    every use is printed as a WIDER line."""
    _, _, g64, e32, pg32, _ = _ORACLES[name]
    bad = []
    for k, v in errors(g, g64).items():
        print(f"[{name}] {k:8s} e32 = {e32[k]}  krn = {v}")
        if v is None:
            assert not np.asarray(g[k]).any(), f"{k}: the oracle's gradient is identically zero"
            continue
        for m, metric in enumerate(("max", "l2")):
            if v[m] <= TOL_FACTOR * e32[k][m]:
                continue
            for stage, back in (("pixel orders", False), ("T from the back", True)):
                y = max([e32[k][m]] + [o[0][k][m] for o in orders(name, back)])
                assert y <= E32_CEILING, f"{name}: the yardstick of {k} {metric} is {y:.2e}: the fp32 statement is broken"
                ok = v[m] <= TOL_FACTOR * y
                if ok or back:
                    print(f"[{name}] WIDER per-tensor {k} {metric}: krn = {v[m]:.3e}  row-by-row e32 = {e32[k][m]:.3e}  "
                          f"{stage} e32 = {y:.3e}  ratio = {v[m] / y:.2f}")
                if ok:
                    break
            else:
                bad.append((k, metric, v[m], e32[k][m], y))
    for k, v in per_gaussian(g, g64).items():
        if v is None:
            assert not np.asarray(g[k]).any(), f"{k}: the oracle's gradient is identically zero"
            continue
        e = v[0]
        y0 = float(pg32[k][0].max())
        i = int(np.argmax(e))
        print(f"[{name}] per-Gaussian {k:8s} e32 = {y0:.3e}  krn = {e[i]:.3e}  ratio = {e[i] / max(y0, 1e-300):.2f}  (worst id {i})")
        for i in np.nonzero(e > TOL_FACTOR * y0)[0]:
            for stage, back in (("pixel orders", False), ("T from the back", True)):
                y = max([y0] + [float(o[1][k][0][i]) for o in orders(name, back)])
                assert y <= E32_CEILING, f"{name}: the yardstick of {k}[{i}] is {y:.2e}: the fp32 statement is broken"
                ok = e[i] <= TOL_FACTOR * y
                if ok or back:
                    print(f"[{name}] WIDER per-Gaussian {k} id {i}: krn = {e[i]:.3e}  row-by-row e32 = {y0:.3e}  "
                          f"{stage} e32 of this Gaussian = {y:.3e}  ratio = {e[i] / y:.2f}  n_i / S = {v[1][i] / v[2]:.2e}")
                if ok:
                    break
            else:
                bad.append((k, int(i), e[i], y0, y))
    assert not bad, f"{name}: beyond {TOL_FACTOR} x the fp32 statement's error, row by row and in every other evaluation: {bad}"


def run_and_judge(be, key, build, **kw):
    c, w, g64, e32, pg32, aux = oracle_of(key, build, **kw)
    g, radii, _, _ = hip_grads(be, c, w, nan_fill=True)
    for k, v in g.items():
        if v is not None:
            assert np.isfinite(v).all(), f"{k}: not fully written"
            assert not v[radii == 0].any(), f"{k}: non-zero gradient for a culled Gaussian"
    judge(key, g)
    return c, w, g, g64, aux


def centre_statement(c, w):
    (g,), _, _ = dgs.grads(c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"], [w], torch.float64)
    return g


# ---- degenerate Gaussians -----------------------------------------------------------------------------------------------------
def test_fronto_parallel_discs(backend):
    """identity quaternion, identity camera, thickness 1e-3: t = z_c on every pixel, strictly inside (lo, hi) = z_c -+ 4e-3, so
    every (instance, pixel) takes the quotient; the depth is the centre's, its derivative by the rotation is not"""
    c, w, g64, _, _, aux = oracle_of("fronto", functools.partial(fronto_case, 1e-3))
    vis = aux["radii"] > 0
    assert aux["quotient_of"][vis].min() > 0 and not aux["clamped"].any() and not aux["fallback"].any()
    gc = centre_statement(c, w)
    assert np.abs(g64["rot"] - gc["rot"]).max() > 0.05 * np.abs(g64["rot"]).max(), "the ray depth turns a fronto-parallel disc"
    run_and_judge(backend, "fronto", None)


def test_isotropic_gaussian_depth_ignores_a_common_scale_and_a_turn(backend):
    """B = s^4 R R^T = s^4 I: t* = (mu . r) / (r . r) whatever the COMMON scale s and the rotation are, and one Gaussian alone has
    D = z_j(p), so with wD and wM alone the depth reaches scale and rotation through the shape of B only.  What vanishes is the
    derivative along a common scaling, s . dL/ds, and along every turn, the part of dL/dq tangent to the unit sphere; one scale
    on its own makes B anisotropic and moves t*, and so does the length of q (R(q) is taken as given: R(c q) = I + c^2 (R(q) - I)
    is no rotation), so dL/ds_k and q . dL/dq do not vanish -- the statement says so, and the kernels are held to it."""
    c, w, g64, e32, pg32, aux = oracle_of("isotropic", isotropic_case)
    assert aux["quotient_of"][0] > 100 and not aux["clamped"].any()
    run_and_judge(backend, "isotropic", None)
    _, wd, gd64, _, _, _ = oracle_of("isotropic/depth", isotropic_case, terms=("wD", "wM"))
    s0 = np.asarray(c["arrays"]["scales"], np.float64)[0]
    q0 = np.asarray(c["arrays"]["rotations"], np.float64)[0]
    tangent = lambda v: v - q0 * (v @ q0) / (q0 @ q0)
    big = np.abs(gd64["scale"]).max()
    assert big > 0 and np.abs(gd64["rot"] @ q0).max() > 0, "one scale alone and the length of q do move the depth"
    assert abs(gd64["scale"][0] @ s0) <= 1e-9 * big * s0[0]
    # the fp32 quaternion is of unit length to 2^-24 only: R R^T - I, and with it the tangent part, is of that order
    assert np.abs(tangent(gd64["rot"][0])).max() <= 1e-6 * np.abs(gd64["rot"]).max()
    _, _, g, _, _ = run_and_judge(backend, "isotropic/depth", None, terms=("wD", "wM"))
    # in fp32 each vanishes to the rounding of its three (four) terms, every one within the bar of its own size
    assert abs(g["scale"][0].astype(np.float64) @ s0) <= 1e-4 * big * s0[0]
    assert np.abs(tangent(g["rot"][0].astype(np.float64))).max() <= 1e-4 * np.abs(gd64["rot"]).max()


def test_rank_one_and_zero_are_the_centre_backward_bit_for_bit(backend):
    """needles and points: w = c = 0, den = 0, every z_j(p) is the fallback z_c -- h goes to row[9] as in the centre backward and
    the second rows stay zero.  The points (all scales 0) have sum s_k^2 M[2][k]^2 = 0: the statement's square-root guard keeps
    it finite, and t = lo = hi there"""
    c, w, g64, e32, pg32, aux = oracle_of("rank1", rank1_case)
    vis = aux["radii"] > 0
    assert aux["fallback_of"][:40].sum() > 0 and aux["fallback_of"][40:].sum() > 0
    assert aux["quotient_of"].sum() == 0 and aux["clamp_hi_of"].sum() == 0 and aux["clamp_lo_of"].sum() == 0
    assert all(np.isfinite(v).all() for v in g64.values() if v is not None), "the square-root guard"
    assert not np.asarray(c["arrays"]["scales"])[40:].any() and vis[40:].any()
    _, _, g, _, _ = run_and_judge(backend, "rank1", None)
    centre, _, _, _ = hip_grads(backend, c, w, ray=False)
    for k in g:
        if g[k] is not None:
            assert g[k].tobytes() == centre[k].tobytes(), k


# ---- the clamps ---------------------------------------------------------------------------------------------------------------
def near_edge_on_case(zc, slab=True):
    """32 x 32, focal 40: Gaussian 0 is a disc (in-plane sigma 0.6 world units, thickness 0, opacity 0.99) centred on the optical
    axis at depth zc whose normal is (cos phi, 0, sin phi), sin phi = 0.02: seen through the 0.3 px dilation alone, as a column.
    Its plane meets the ray of column rx at t = 0.02 zc / (rx cos phi + 0.02); the four columns that contribute have
    rx = -+0.0125, -+0.0375:  t = -1.1 zc (below lo), 2.7 zc (above hi = zc + 2.4 for zc = 3), 0.62 zc and 0.35 zc.
    ``slab``: behind it a slab of thickness 1e-3 at z = 5 covers the image."""
    W = H = 32
    f = 40.0
    rng = np.random.default_rng(917)
    phi = np.arcsin(0.02)
    th = 0.5 * np.pi - phi           # R_y(th): local z -> (sin th, 0, cos th) = (cos phi, 0, sin phi)
    xyz = np.array([[0.0, 0.0, zc], [0.0, 0.0, 5.0]])
    s = np.array([[0.6, 0.6, 0.0], [8.0, 8.0, 1e-3]])
    q = np.array([[np.cos(th / 2), 0.0, np.sin(th / 2), 0.0], IDENT])
    n = 2 if slab else 1
    return finish(f"near_edge_on{zc}", xyz[:n], s[:n], q[:n], [0.99, 0.7][:n], random_shs(rng, n), W, H, f)


def test_edge_on_disc_clamped_at_hi_and_at_lo(backend):
    """both clamps bind on the disc, each on a column of its own: h goes to dL/dz_c and +-4 h to dL/dsz, which reaches the
    in-plane scale that spans the view axis and the rotation"""
    c, w, g64, _, _, aux = oracle_of("clamp_hi_lo", functools.partial(near_edge_on_case, 3.0))
    assert aux["clamp_hi_of"][0] >= 8 and aux["clamp_lo_of"][0] >= 8 and aux["floor_of"][0] == 0
    assert aux["clamp_hi_of"][1] == aux["clamp_lo_of"][1] == 0 and aux["quotient_of"][1] > 500
    # what the clamps alone send to the scales: the same loss with the centre's z has no such term
    gc = centre_statement(c, w)
    assert np.abs(g64["scale"][0] - gc["scale"][0]).max() > 0.05 * np.abs(g64["scale"][0]).max()
    run_and_judge(backend, "clamp_hi_lo", None)


def test_disc_clamped_at_the_floor_gets_no_depth_gradient(backend):
    """the same disc alone at z_c = 0.5: lo = max(0.5 - 2.4, 0.2) is the floor and hi = 2.9; the columns left of the middle two meet the plane
    behind the camera and are clamped to 0.2, where the depth is a constant"""
    c, w, g64, _, _, aux = oracle_of("floor", functools.partial(near_edge_on_case, 0.5, False), terms=("wD", "wM"))
    assert aux["floor_of"][0] >= 8 and aux["clamp_lo_of"][0] == 0, "the clamp that binds below is the floor"
    run_and_judge(backend, "floor", None, terms=("wD", "wM"))
    # the floor-clamped columns alone: weights elsewhere zero.  One Gaussian: D = z_j(p) = 0.2 exactly, no path is left
    cols = np.zeros((c["H"], c["W"]), bool)
    cols[:, :c["W"] // 2 - 1] = True      # rx <= -0.0375: behind the camera; column 15 (rx = -0.0125) meets the plane at 2.7 z_c
    wf = {k: np.where(cols, v, np.float32(0)) for k, v in w.items()}
    (gf,), _, auxf = rdgs.grads(c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"], [wf], torch.float64)
    on = (auxf["n_contrib"] > 0) & cols
    assert on.sum() >= 8 and auxf["floor_clamped"][on].all(), "every contributing pixel left of the middle columns is clamped at the floor"
    scale = float(sum(np.abs(v).sum() for v in wf.values()))
    for k in ("mean3D", "scale", "rot", "opacity"):
        assert np.abs(gf[k]).max() <= 1e-12 * scale, f"statement: {k}"
    g, _, _, _ = hip_grads(backend, c, wf)
    # D = fmaf(w, 0.2f, 0) / w differs from 0.2f by at most one rounding, so |u| <= 2^-23 0.2 |gD| / S reaches alpha: what is
    # left is of that order, against gradients of order |gD| where the clamp does not bind
    print(f"[floor] floor-clamped columns alone: max |mean3D| {np.abs(g['mean3D']).max():.2e} |scale| {np.abs(g['scale']).max():.2e} "
          f"|rot| {np.abs(g['rot']).max():.2e} against sum |w| = {scale:.2e}")
    for k in ("mean3D", "scale", "rot"):
        assert np.abs(g[k]).max() <= 1e-5 * scale, f"{k}: a depth clamped at the floor passed a gradient"


# ---- lists and image sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_tilted_stack_crosses_the_batch_boundaries(backend, n):
    c, w, g64, _, _, aux = oracle_of(f"ray_stack{n}", functools.partial(stack_case, n))
    assert aux["tile_len"].tolist() == [[n]] and aux["n_contrib"].max() == n, "the centre pixel meets all n"
    assert (aux["quotient_of"] > 0).all(), "every record of the list is read at a quotient"
    assert (np.abs(g64["rot"]).max(axis=1) > 0).all()
    run_and_judge(backend, f"ray_stack{n}", None)


@pytest.mark.parametrize("W,H", [(1, 1), (15, 15), (17, 17)])
def test_images_below_a_tile_and_one_pixel_over(backend, W, H):
    c, w, g64, _, _, aux = oracle_of(f"size{W}x{H}", functools.partial(size_case, W, H))
    assert aux["tile_len"].shape == ((H + 15) // 16, (W + 15) // 16) and aux["tile_len"].min() > 0
    assert (aux["n_contrib"] > 0).all(), "Gaussian 0 covers every pixel"
    if W > 16:
        rect = aux["rect"].astype(np.int64)
        assert ((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).max() == 4, "second rows summed over four slots"
    run_and_judge(backend, f"size{W}x{H}", None)


# ---- large and non-finite input -----------------------------------------------------------------------------------------------
def test_ids_beyond_65536(backend):
    """the scan scene of the backward's edge tests: the compact scene holds the visible Gaussians of the big one in the same
    order, so their gradients are the same bits, and the ray records and second rows are indexed by ids up to 131 700"""
    big, compact, ids = scan_scenes()
    assert ids.max() >= 131072
    c, w, g, g64, aux = run_and_judge(backend, "scan", lambda: compact)
    assert aux["quotient_of"][ids >= 65536].sum() > 0
    gb, _, _, _ = hip_grads(backend, big, w)
    for k in g:
        if g[k] is not None:
            assert gb[k][ids].tobytes() == g[k].tobytes(), k
            rest = np.ones(gb[k].shape[0], bool)
            rest[ids] = False
            assert not gb[k][rest].any(), k


def test_infinite_scale_keeps_to_its_own_rows(backend):
    """case 8 of tests/test_raster_depth_ray_edges.py: Gaussian 0 (scales (0.1, inf, 0.1)) is listed on every tile with a NaN
    conic and alpha 0.99 on EVERY pixel, in front of everything, at the fallback depth z_c.  Its own gradients are not finite (G
    is NaN); every OTHER Gaussian's are, and they do not depend on what its non-finite values are: a second run with another
    infinite axis gives them the same bits.  (They are NOT those of the scene without it -- it takes every pixel's T to 0.01
    before anything else is seen -- and the statement cannot say what they are: its walk drops an instance whose power is NaN,
    the kernels' keeps it.)"""
    c = infinite_scale_case()
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(5)
    w = {k: rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32) for k in ("wD", "wM", "wA")}
    w["wC"] = rng.uniform(-1.0, 1.0, (3, H, W)).astype(np.float32)
    g, radii, _, _ = hip_grads(backend, c, w, nan_fill=True)
    assert radii[0] == 2 ** 31 - 1 and (radii[1:] > 0).all()
    for k, v in g.items():
        if v is not None:
            assert np.isfinite(v[1:]).all(), f"{k}: the infinite scale reached another Gaussian"
    assert np.abs(g["rot"][1:]).max() > 0 and np.abs(g["scale"][1:]).max() > 0
    s2 = np.array(c["arrays"]["scales"])
    s2[0] = [0.1, np.inf, np.inf]
    g2, radii2, _, _ = hip_grads(backend, dict(c, arrays=dict(c["arrays"], scales=s2)), w)
    if radii2[0] == radii[0]:          # listed the same way: the same lists, the same front layer
        for k, v in g.items():
            if v is not None:
                assert v[1:].tobytes() == g2[k][1:].tobytes(), k


# ---- error paths --------------------------------------------------------------------------------------------------------------
def test_errors_return_the_code_and_write_nothing(backend):
    c = big_case("small800")
    w = {"wD": np.ones((c["H"], c["W"]), np.float32)}
    with pytest.raises(RuntimeError, match="gs2m_rasterize_backward_depth_ray: the handle holds no state"):
        hip_grads(backend, c, w, forward=False)
    _, _, r, _ = hip_grads(backend, c, w)
    with pytest.raises(RuntimeError, match="do not match"):
        hip_grads(backend, dict(c, W=c["W"] - 1), {"wD": np.ascontiguousarray(w["wD"][:, 1:])}, r=r, forward=False)
    # a forward that took cov3D_precomp has no ray depth; through the C entry itself: the error code, and nothing written
    p = big_case("precomp")
    d = backend.dev
    a, cam = p["arrays"], p["cam"]
    xyz, cov, col = d(a["means3D"]), d(a["cov3D_precomp"]), d(a["colors_precomp"])
    vm, pm, cp, bg = d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(p["bg"])
    P = a["means3D"].shape[0]
    outs = [d(np.full(s, 7.0, np.float32)) for s in ((P, 3), (P, 4), (P,), (P, 3), (P, 3), (P, 6), (P, 3), (P, 4))]
    ptr, st = _lib._ptr, _lib._stream_of(xyz, None)
    s_, q_, gD = d(c["arrays"]["scales"]), d(c["arrays"]["rotations"]), d(w["wD"])

    def entry(r, sc, ro, cv, width):
        rc = backend.lib.gs2m_rasterize_backward_depth_ray(
            r._h, P, 3, 0, 0, ptr(bg), width, p["H"], ptr(xyz), None, ptr(col), ptr(sc), 1.0, ptr(ro), ptr(cv), ptr(vm), ptr(pm),
            ptr(cp), cam.tanfovx, cam.tanfovy, None, ptr(gD), None, None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
            ptr(outs[3]), ptr(outs[4]), ptr(outs[5]), None, ptr(outs[6]), ptr(outs[7]), 0, st)
        backend.sync()
        for o in outs:
            assert (backend.host(o) == 7.0).all(), "an error writes nothing"
        return rc

    r = Rasterizer(0, lib=backend.lib)
    assert entry(r, s_, q_, None, p["W"]) == 1 and b"no state" in backend.lib.gs2m_last_error()
    r.forward(xyz, d(a["opacities"]), vm, pm, cp, bg, p["W"], p["H"], cam.tanfovx, cam.tanfovy, colors_precomp=col, cov3D_precomp=cov)
    assert entry(r, None, None, cov, p["W"]) == 1 and b"cov3D_precomp has no ray depth" in backend.lib.gs2m_last_error()
    for sc, ro, cv in ((s_, q_, cov), (s_, None, None), (None, q_, None)):
        assert entry(r, sc, ro, cv, p["W"]) == 1
    assert entry(r, s_, q_, None, p["W"] + 1) == 1 and b"do not match" in backend.lib.gs2m_last_error()
    with pytest.raises(RuntimeError, match="ray depth"):
        hip_grads(backend, p, w, r=r, forward=False)
