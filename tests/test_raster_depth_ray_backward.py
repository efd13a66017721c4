"""Gradients through the ray-Gaussian intersection depth maps (gs2m_rasterize_backward_depth_ray) against the differentiable fp64
statement tests/ray_depth_grad_statement.py: depth_grad_statement.py with z_j(p) of ray_depth_statement.py over leaf tensors.

Loss: that of tests/test_raster_depth_backward.py on the ray maps, sum(wC image + wD expected_ray + wM median_ray + wA alpha), with
the same seeded weights.  Every weight is zero on a pixel in one of these sets, all found on the fp64 statement alone, each with a
cap that is asserted:
    threshold   a decision of renderCUDA within 1e-4 of its threshold (test_raster_backward.case)                   <= 1 %
    near05      a transmittance within 1e-4 of 0.5 -- wM only (with threshold, as test_raster_depth_backward)      <= 1 %
    grazing     a contributor with a weight > 0 meets the ray within ~1.8 degrees of its plane (GRAZING_CAP)        <= 10 %
    near clamp  a contributor with a weight > 0 has t within 1e-4, relative, of lo or hi                            <= 2 %
Shares on the statement (printed with -s): small800 grazing 0 %, near a clamp 0.013 %; ragged3000 0 % and 0 %; trained grazing
5.8 %, near a clamp 0.85 %, and 27 % of its pixels have a clamped contributor, 9.5 % one clamped at the 0.2 floor: the clamp
branches of the derivative run (asserted: > 5 %).

Tolerance (per gradient tensor, max|g - g64| / max|g64| and relative L2): TOL_FACTOR = 4 x the error of the SAME statement
evaluated in fp32 -- test_raster_backward.check, the project's bar.  Measured figures: profiles/raster_depth_ray_backward.txt.
"""
import functools

import numpy as np
import pytest
import torch

import depth_grad_statement as dgs
import ray_depth_grad_statement as rdgs
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_backward import case, check, errors
from test_raster_depth_backward import ALONE, weights_of
from test_raster_depth_ray import GRAZING_CAP, tilted_plane_case

CASES = ["small800", "ragged3000", "trained"]
NEAR_CLAMP_CAP = 0.02


def masked_sets(name, base, near, alone):
    """-> a function aux -> weight sets for rdgs.grads: ``base`` (wC, wD, wM, wA) with the exclusions of the module docstring
    applied from the flags of the fp64 evaluation; asserts their caps.  What it returned is kept in .sets"""
    def build(aux):
        off = near | aux["grazing"] | aux["near_clamp"]
        shares = {k: float(aux[k].mean()) for k in ("grazing", "near_clamp", "clamped", "floor_clamped", "fallback", "near05")}
        print(f"[{name}] statement shares: threshold {near.mean():.3%}, " + ", ".join(f"{k} {v:.3%}" for k, v in shares.items()))
        assert near.mean() <= 0.01, f"{name}: {near.mean():.2%} of the pixels sit on a threshold"
        assert (near | aux["near05"]).mean() <= 0.01, f"{name}: {aux['near05'].mean():.2%} of the pixels have T near 0.5"
        assert shares["grazing"] <= GRAZING_CAP, f"{name}: {shares['grazing']:.2%} of the pixels have a grazing contributor"
        assert shares["near_clamp"] <= NEAR_CLAMP_CAP, f"{name}: {shares['near_clamp']:.2%} of the pixels sit near a clamp"
        w = {k: np.where(off[None] if v.ndim == 3 else off, np.float32(0), v) for k, v in base.items()}
        if "wM" in w:
            w["wM"] = np.where(aux["near05"], np.float32(0), w["wM"])
        build.sets = [w] + ([{v: w[v]} for v in ALONE.values()] if alone else [])
        build.shares = shares
        return build.sets
    return build


def oracle_for(c, name, base, near, alone=False):
    """-> (weight sets, g64 per set, e32 per set, aux of the fp64 run, shares)"""
    args = (c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    build = masked_sets(name, base, near, alone)
    g64, _, aux = rdgs.grads(*args, build, torch.float64)
    g32, _, _ = rdgs.grads(*args, build.sets, torch.float32)
    return build.sets, g64, [errors(x, y) for x, y in zip(g32, g64)], aux, build.shares


@functools.lru_cache(maxsize=None)
def oracle_of(name, alone=False):
    w, near = weights_of(name)
    out = oracle_for(case(name), name, w, near, alone)
    aux = out[3]
    assert (aux["median_pos"] > 0).mean() > 0.1 and (aux["n_contrib"] > 0).mean() > 0.3, "the scene must exercise the maps"
    return out


def hip_grads(be, c, w, ray=True, twice=False, maps_between=False, nan_fill=False, r=None, forward=True, lib=None):
    """w: dict with any of wC, wD, wM, wA.  -> (gradients as numpy, radii, Rasterizer, ray maps before / after the backward)"""
    import gs2mesh_amd.rasterizer as rz
    a, d, cam = c["arrays"], be.dev, c["cam"]
    r = r or Rasterizer(0, lib=lib or be.lib)
    dev = {k: d(v) for k, v in a.items() if k not in ("means3D", "opacities")}
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"],
              cam.tanfovx, cam.tanfovy)
    xyz = d(a["means3D"])
    radii = None
    if forward:
        _, radii = r.forward(xyz, d(a["opacities"]), *common, sh_degree=c["deg"], scale_modifier=c["mod"], **dev)
    ray_maps = lambda: {k: be.host(v).copy() for k, v in r.depth_maps_ray(
        xyz, dev["scales"], dev["rotations"], common[0], c["W"], c["H"], cam.tanfovx, cam.tanfovy, scale_modifier=c["mod"]).items()}
    before = ray_maps() if maps_between else None
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):      # NaN-filled outputs: every element must be written
        t = real_empty(like, shape, np_dtype)
        if np_dtype == np.float32:
            t[...] = float("nan")
        return t

    outs = []
    rz._empty = nan_empty if nan_fill else real_empty
    try:
        for _ in range(2 if twice else 1):
            g = r.backward(d(w.get("wC")), xyz, *common, sh_degree=c["deg"], scale_modifier=c["mod"], want_conic=True,
                           grad_depth=d(w.get("wD")), grad_median=d(w.get("wM")), grad_alpha=d(w.get("wA")), ray_depth=ray, **dev)
            be.sync()
            outs.append({k: (None if v is None else be.host(v).copy()) for k, v in g.items()})
    finally:
        rz._empty = real_empty
    after = ray_maps() if maps_between else None
    return (outs if twice else outs[0]), (None if radii is None else be.host(radii)), r, (before, after)


@pytest.mark.parametrize("name", CASES)
def test_gradients_through_image_and_ray_maps_match_the_statement(backend, name):
    c = case(name)
    sets, g64, e32, aux, shares = oracle_of(name, alone=name == "small800")
    if name == "trained":
        assert shares["clamped"] > 0.05, "the clamp branches of the derivative must run in this scene"
        assert aux["clamp_hi_of"].sum() > 0 and aux["clamp_lo_of"].sum() > 0 and aux["floor_of"].sum() > 0
    P = c["arrays"]["means3D"].shape[0]
    g, radii, _, _ = hip_grads(backend, c, sets[0], nan_fill=True)
    np.testing.assert_array_equal(radii, aux["radii"])
    for k, v in g.items():
        if v is not None:
            assert v.shape[0] == P and np.isfinite(v).all(), f"{k}: not fully written"
            assert not v[radii == 0].any(), f"{k}: non-zero gradient for a culled Gaussian"
    assert (radii == 0).any() or name != "ragged3000"
    assert not g["mean2D"][:, 2].any()
    check(f"ray/{name}", g, g64[0], e32[0])


@pytest.mark.parametrize("which", list(ALONE))
def test_each_upstream_gradient_alone(backend, which):
    """one map's gradient, the other two and dL_dpix NULL"""
    c = case("small800")
    sets, g64, e32, _, _ = oracle_of("small800", alone=True)
    i = 1 + list(ALONE).index(which)
    assert list(sets[i]) == [ALONE[which]]
    g, _, _, _ = hip_grads(backend, c, sets[i])
    assert not g["color"].any() and not g["sh"].any(), "no colour term in this loss"
    if which in "DM":
        assert np.abs(g64[i]["rot"]).max() > 0 and np.abs(g64[i]["scale"]).max() > 0, "the ray depth reaches rotation and scale"
    check(f"ray alone/{which}", g, g64[i], e32[i])


def test_without_a_depth_gradient_the_call_is_the_centre_backward_bit_for_bit(backend):
    c = case("ragged3000")
    w, _ = weights_of("ragged3000")
    for keys in (("wC", "wA"), ("wA",), ("wC",)):
        sub = {k: w[k] for k in keys}
        ray, _, _, _ = hip_grads(backend, c, sub)
        centre, _, _, _ = hip_grads(backend, c, sub, ray=False)
        for k in ray:
            if ray[k] is not None:
                assert ray[k].tobytes() == centre[k].tobytes(), (keys, k)


def test_two_calls_give_identical_bits(backend):
    sets, _, _, _, _ = oracle_of("small800", alone=True)
    (g1, g2), _, _, _ = hip_grads(backend, case("small800"), sets[0], twice=True)
    for k in g1:
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k


def test_the_backward_leaves_the_ray_maps_alone_and_reports_its_rows(backend):
    """forward -> depth_maps_ray -> backward: the maps' bits are unchanged, and the gradients are those of a backward without the
    maps call; the row count and the first arena are what the centre backward reports"""
    c = case("small800")
    sets, _, _, _, _ = oracle_of("small800", alone=True)
    g1, _, r1, (before, after) = hip_grads(backend, c, sets[0], maps_between=True)
    g2, _, r2, _ = hip_grads(backend, c, sets[0])
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for k in g1:
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k
    _, _, r3, _ = hip_grads(backend, c, sets[0], ray=False)
    assert r1.backward_rows() == r3.backward_rows()


# ---- what the derivative is for: a depth residual turns a flat Gaussian --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tilted_oracle():
    c, _ = tilted_plane_case()
    near = c["w"][0] == 0
    wD = np.random.default_rng(4321).uniform(-1.0, 1.0, (c["H"], c["W"])).astype(np.float32)
    return (c,) + oracle_for(c, "tilted_plane", {"wD": wD}, near)


def test_depth_gradient_turns_the_discs_of_a_tilted_plane(backend):
    """loss = sum(wD expected_ray) alone on the 60 degree plane of flat discs: in the fp64 statement dL_drot is non-zero on at
    least half of the visible discs and the operator matches it within the bar; the centre backward of the same loss on the
    centre map reaches rotation through alpha alone, and agrees with it on no disc"""
    c, sets, g64, e32, aux, _ = tilted_oracle()
    vis = aux["radii"] > 0
    rot64 = np.abs(g64[0]["rot"]).max(axis=1)
    turning = vis & (rot64 > 1e-6 * rot64.max())
    assert turning.sum() >= 0.5 * vis.sum(), f"dL_drot is non-zero on {turning.sum()} of {vis.sum()} visible discs"
    g, _, _, _ = hip_grads(backend, c, sets[0])
    check("ray/tilted_plane", g, g64[0], e32[0])
    centre, _, _, _ = hip_grads(backend, c, sets[0], ray=False)
    diff = np.abs(centre["rot"] - g["rot"]).max(axis=1)
    scale = np.abs(g["rot"]).max(axis=1)
    print(f"[tilted plane] discs that turn: {turning.sum()} of {vis.sum()}; min over them of |rot_centre - rot_ray| / |rot_ray| = "
          f"{(diff[turning] / scale[turning]).min():.3f}")
    assert (diff[turning] > 0.01 * scale[turning]).all(), "the centre backward agrees with the ray backward on some disc"
    # and the centre statement confirms what the centre backward computed: it is a different function, not an error
    g64c, _, _ = dgs.grads(c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"], sets, torch.float64)
    assert np.abs(g64c[0]["rot"] - g64[0]["rot"]).max() > 0.1 * np.abs(g64[0]["rot"]).max()
