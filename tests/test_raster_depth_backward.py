"""Gradients through the depth and opacity maps (gs2m_rasterize_backward_depth) against the differentiable fp64 statement
tests/depth_grad_statement.py: raster_statement.py's projection feeding depth_statement.py's walk.

Loss: sum(wC image + wD depth_expected + wM depth_median + wA alpha) with fixed seeded weights in [-1, 1).  Every weight is zero
on pixels where the oracle's replay of renderCUDA finds a decision within 1e-4 of its threshold (oracle.render_flip_bounds, as
test_raster_backward.py does); wM is also zero where a transmittance lies within 1e-4 of 0.5 (the median may then be another
instance in fp32).  At most 1 % of the pixels may be zeroed, asserted from the fp64 statement alone.

Tolerance (per gradient tensor, max|g - g64| / max|g64| and relative L2): TOL_FACTOR = 4 x the error of the SAME statement
evaluated in fp32 -- the project's bar for the colour backward (test_raster_backward.py), independent of the code under test.
Measured figures: profiles/raster_depth_backward.txt.
"""
import functools

import numpy as np
import pytest

import depth_grad_statement as dgs
import depth_statement
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_backward import case, check, errors

CASES = ["small800", "trained", "ragged3000", "precomp"]
ALONE = {"D": "wD", "M": "wM", "A": "wA"}


@functools.lru_cache(maxsize=None)
def weights_of(name):
    """-> (all four weights, near, near05-independent parts); wM still has to be masked by near05 (oracle_of does)"""
    c = case(name)
    near = c["w"][0] == 0       # case() zeroed its colour weights exactly there (a drawn weight of exactly 0 only adds to the share)
    rng = np.random.default_rng(1234)
    w = {k: rng.uniform(-1.0, 1.0, (c["H"], c["W"])).astype(np.float32) for k in ("wD", "wM", "wA")}
    for v in w.values():
        v[near] = 0.0
    w["wC"] = c["w"]
    return w, near


@functools.lru_cache(maxsize=None)
def oracle_of(name, alone=False):
    """-> (weight sets, g64 per set, e32 per set, aux of the fp64 run).  Set 0 is the full loss; with ``alone`` sets 1..3 are wD,
    wM and wA on their own (no colour term)."""
    c = case(name)
    w, near = weights_of(name)
    a = c["arrays"]
    args = (a, c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    import torch
    aux0 = depth_statement.depth_maps(a, c["cam"], c["W"], c["H"], c["mod"])   # the fp64 walk: where a T sits at 0.5
    w = dict(w, wM=np.where(aux0["near05"], np.float32(0), w["wM"]))
    zeroed = float((near | aux0["near05"]).mean())
    assert zeroed <= 0.01, f"{zeroed:.2%} of the pixels sit on a threshold"
    sets = [w] + ([{v: w[v]} for v in ALONE.values()] if alone else [])
    g64, maps64, aux = dgs.grads(*args, sets, torch.float64)
    g32, _, _ = dgs.grads(*args, sets, torch.float32)
    assert (aux["median_pos"] > 0).mean() > 0.1 and (aux["n_contrib"] > 0).mean() > 0.3, "the scene must exercise the maps"
    return sets, g64, [errors(x, y) for x, y in zip(g32, g64)], aux


class ViaDepthEntry:
    """a bound library whose gs2m_rasterize_backward IS gs2m_rasterize_backward_depth with the three new pointers NULL"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def gs2m_rasterize_backward(self, *a):
        return self._lib.gs2m_rasterize_backward_depth(*a[:21], None, None, None, *a[21:])


class NullPix(ViaDepthEntry):
    """gs2m_rasterize_backward -> gs2m_rasterize_backward_depth with all four upstream pointers NULL"""

    def gs2m_rasterize_backward(self, *a):
        return self._lib.gs2m_rasterize_backward_depth(*a[:20], None, None, None, None, *a[21:])


def hip_grads(be, c, w, twice=False, lib=None, rows=1, r=None, forward=True):
    """w: dict with any of wC, wD, wM, wA.  -> (gradients as numpy, radii, Rasterizer)"""
    a = c["arrays"]
    d = be.dev
    cam = c["cam"]
    r = r or Rasterizer(0, lib=lib or be.lib)
    if rows != 1:
        r.set_option(_lib.OPT_TILE_ROWS, rows)
    dev = {k: d(v) for k, v in a.items() if k not in ("means3D", "opacities")}
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"],
              cam.tanfovx, cam.tanfovy)
    xyz = d(a["means3D"])
    radii = None
    if forward:
        _, radii = r.forward(xyz, d(a["opacities"]), *common, sh_degree=c["deg"], scale_modifier=c["mod"], **dev)
    outs = []
    for _ in range(2 if twice else 1):
        g = r.backward(d(w.get("wC")), xyz, *common, sh_degree=c["deg"], scale_modifier=c["mod"], want_conic=True,
                       grad_depth=d(w.get("wD")), grad_median=d(w.get("wM")), grad_alpha=d(w.get("wA")), **dev)
        be.sync()
        outs.append({k: (None if v is None else be.host(v).copy()) for k, v in g.items()})
    return (outs if twice else outs[0]), (None if radii is None else be.host(radii)), r


@pytest.mark.parametrize("name", CASES)
def test_gradients_through_image_and_maps_match_the_statement(backend, name):
    c = case(name)
    sets, g64, e32, aux = oracle_of(name, alone=name == "small800")
    if name == "trained":
        assert aux["capped"] >= 1, "the 0.99 cap must bind in this scene"
    P = c["arrays"]["means3D"].shape[0]
    import gs2mesh_amd.rasterizer as rz
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):      # NaN-filled outputs: every element must be written
        t = real_empty(like, shape, np_dtype)
        if np_dtype == np.float32:
            t[...] = float("nan")
        return t

    rz._empty = nan_empty
    try:
        g, radii, _ = hip_grads(backend, c, sets[0])
    finally:
        rz._empty = real_empty
    np.testing.assert_array_equal(radii, aux["radii"])
    for k, v in g.items():
        if v is not None:
            assert v.shape[0] == P and np.isfinite(v).all(), f"{k}: not fully written"
            assert not v[radii == 0].any(), f"{k}: non-zero gradient for a culled Gaussian"
    assert (radii == 0).any() or name != "ragged3000"
    assert not g["mean2D"][:, 2].any()
    check(f"depth/{name}", g, g64[0], e32[0])


@pytest.mark.parametrize("which", list(ALONE))
def test_each_upstream_gradient_alone(backend, which):
    """one map's gradient, the other two and dL_dpix NULL: a term leaking into another's path shows here"""
    c = case("small800")
    sets, g64, e32, _ = oracle_of("small800", alone=True)
    i = 1 + list(ALONE).index(which)
    assert list(sets[i]) == [ALONE[which]]
    g, _, _ = hip_grads(backend, c, sets[i])
    assert not g["color"].any() and not g["sh"].any(), "no colour term in this loss"
    if which == "A":
        assert np.abs(g64[i]["mean3D"]).max() > 0
    check(f"alone/{which}", g, g64[i], e32[i])


def test_colour_only_call_is_the_colour_backward_bit_for_bit(backend):
    """the new entry with its three new pointers NULL runs the colour kernels: the bits of gs2m_rasterize_backward, -0 included"""
    c = case("ragged3000")
    old, _, _ = hip_grads(backend, c, {"wC": c["w"]})
    new, _, _ = hip_grads(backend, c, {"wC": c["w"]}, lib=ViaDepthEntry(backend.lib))
    for k in old:
        if old[k] is not None:
            assert old[k].tobytes() == new[k].tobytes(), k
    # and the depth kernels with zero maps compute the same colour gradients up to the sign of a zero
    zero = np.zeros((c["H"], c["W"]), np.float32)
    dep, _, _ = hip_grads(backend, c, {"wC": c["w"], "wD": zero, "wM": zero, "wA": zero})
    for k in old:
        if old[k] is not None:
            np.testing.assert_array_equal(old[k], dep[k], err_msg=k)


def test_depth_backward_is_bitwise_reproducible(backend):
    sets, _, _, _ = oracle_of("small800", alone=True)
    (g1, g2), _, _ = hip_grads(backend, case("small800"), sets[0], twice=True)
    for k in g1:
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k


def test_all_upstream_gradients_null_gives_zeros(backend):
    c = case("small800")
    g, _, _ = hip_grads(backend, c, {}, lib=NullPix(backend.lib))
    for k, v in g.items():
        if v is not None:
            assert not v.any(), k


def test_errors_of_the_colour_backward_are_errors_of_the_depth_backward(backend):
    c = case("small800")
    w = {"wD": np.ones((c["H"], c["W"]), np.float32)}
    with pytest.raises(RuntimeError, match="gs2m_rasterize_backward_depth: the handle holds no state"):
        hip_grads(backend, c, w, forward=False)
    with pytest.raises(RuntimeError, match="TILE_ROWS"):
        hip_grads(backend, c, w, rows=2)
    _, _, r = hip_grads(backend, c, w)
    small = dict(c, arrays={k: (None if v is None else v[:10]) for k, v in c["arrays"].items()})
    with pytest.raises(RuntimeError, match="do not match"):
        hip_grads(backend, small, w, r=r, forward=False)
    with pytest.raises(RuntimeError, match="do not match"):
        hip_grads(backend, dict(c, H=c["H"] - 1), {"wD": w["wD"][1:]}, r=r, forward=False)
    r.set_option(_lib.OPT_PAIR_BATCH, 2)
    with pytest.raises(RuntimeError, match="PAIR_BATCH"):
        hip_grads(backend, c, w, r=r, forward=False)
    # a forward that overflowed its arena (far too small on purpose); its status has reached the host after a sync
    r = Rasterizer(0, lib=backend.lib)
    r.reserve(c["arrays"]["means3D"].shape[0], 1, c["W"], c["H"], 64)
    a, d, cam = c["arrays"], backend.dev, c["cam"]
    r.forward(d(a["means3D"]), d(a["opacities"]), d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center),
              d(c["bg"]), c["W"], c["H"], cam.tanfovx, cam.tanfovy, shs=d(a["shs"]), scales=d(a["scales"]),
              rotations=d(a["rotations"]), sync=False)
    backend.sync()
    with pytest.raises(RuntimeError, match="overflowed"):
        hip_grads(backend, c, w, r=r, forward=False)
    r.status(1)      # consume the sticky overflow word
    # and a NULL dL_dpix stays an error of the colour entry
    with pytest.raises(RuntimeError, match="NULL required pointer"):
        hip_grads(backend, c, {})
