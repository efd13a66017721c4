"""Depth and opacity maps of the rasteriser (gs2m_rasterize_depth, k_blend_depth) against the fp64 statement of the walk
(tests/depth_statement.py), on both back-ends.

Exclusions: pixels where the oracle's replay of renderCUDA finds a decision within 1e-4 of its threshold (the zeroed weights of
test_raster_backward.case: at most 1 % of the pixels) and pixels where some contributor leaves the transmittance within 1e-4,
relative, of 0.5 (``near05``: fp32 and fp64 may pick different medians; at most 0.2 %).

Tolerance on the kept pixels: alpha and depth_expected within TOL_FACTOR (4, the backward's contract: the same bw_alpha, the same
fast exp, the same O(n 2^-24) reordering) x the error of the SAME statement evaluated in fp32 on the CPU, in
max|x - x64| / max|x64| and in relative L2 -- independent of the code under test.  depth_median is bit-equal to the fp32
view-space z (oracle.preprocess) of the statement's median Gaussian, and exactly 0 where the statement has none.
Measured figures: profiles/raster_depth.txt (``-s`` prints them).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import depth_statement as ds
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer
from test_raster_backward import TOL_FACTOR, case

CASES = ["small800", "ragged3000", "trained"]
MAPS = ("expected", "median", "alpha")


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """-> (fp64 statement, e32 = {map: errors of the fp32 statement}, keep[H,W]); asserts the caps on the exclusions, that
    fp32 and fp64 agree on the median's Gaussian on every kept pixel, and that the scene is not vacuous"""
    c = case(name)
    s64 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float64)
    s32 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], c["mod"], torch.float32)
    near = c["w"][0] == 0                      # a renderCUDA decision within 1e-4 of its threshold
    assert c["zeroed"] <= 0.01, f"{name}: {c['zeroed']:.2%} of the pixels sit on a threshold"
    assert s64["near05"].mean() <= 0.002, f"{name}: {s64['near05'].mean():.3%} of the pixels have T within 1e-4 of 0.5"
    keep = ~near & ~s64["near05"]
    np.testing.assert_array_equal(s32["median_id"][keep], s64["median_id"][keep])
    np.testing.assert_array_equal(s32["n_contrib"][keep], s64["n_contrib"][keep])
    has = s64["median_id"] >= 0
    assert has.mean() >= 0.10 and not has.all(), f"{name}: {has.mean():.1%} of the pixels have a median"
    e32 = {k: ds.errors(s32[k], s64[k], keep) for k in ("alpha", "expected")}
    for v in s64.values():
        v.setflags(write=False)
    print(f"[{name}] statement: excluded {near.mean():.3%} (threshold) + {s64['near05'].mean():.3%} (T near 0.5); median on "
          f"{has.mean():.1%} of the pixels, no contributor on {(s64['n_contrib'] == 0).mean():.1%}; e32 alpha = {e32['alpha']}, "
          f"expected = {e32['expected']}")
    return s64, e32, keep


def forward(be, c, cull=0, rows=1, r=None, sync=True):
    """forward of case c on back-end be -> (handle, the device arrays of the call)"""
    a, cam = c["arrays"], c["cam"]
    d = be.dev
    r = r or Rasterizer(0, lib=be.lib)
    r.set_option(_lib.OPT_EXACT_TILE_CULL, cull)
    if rows != 1:
        r.set_option(_lib.OPT_TILE_ROWS, rows)
    dev = {k: d(v) for k, v in a.items() if k not in ("means3D", "opacities")}
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"],
              cam.tanfovx, cam.tanfovy)
    xyz = d(a["means3D"])
    img, _ = r.forward(xyz, d(a["opacities"]), *common, sh_degree=c["deg"], scale_modifier=c["mod"], sync=sync, **dev)
    return r, dict(xyz=xyz, common=common, dev=dev, img=img)


def maps_of(be, r, c, want=MAPS, like=None):
    """depth_maps into NaN-filled buffers -> dict of host copies; every map must come back finite"""
    import gs2mesh_amd.rasterizer as rz
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):
        t = real_empty(like, shape, np_dtype)
        t[...] = float("nan")
        return t

    rz._empty = nan_empty
    try:
        m = r.depth_maps(c["W"], c["H"], want=want, like=like if like is not None else be.dev(np.zeros(1, np.float32)))
        be.sync()
    finally:
        rz._empty = real_empty
    m = {k: be.host(v).copy() for k, v in m.items()}
    for k, v in m.items():
        assert v.shape == (c["H"], c["W"]) and v.dtype == np.float32 and np.isfinite(v).all(), f"{k}: not fully written"
    return m


def hip_maps(be, c, **kw):
    r, _ = forward(be, c, **kw)
    return maps_of(be, r, c), r


def check(name, m, s64, e32, keep, geom_depths):
    """the contract of the module docstring; prints kernel / e32 per map and metric"""
    bad = []
    for k, hip in (("alpha", m["alpha"]), ("expected", m["expected"])):
        e = ds.errors(hip, s64[k], keep)
        print(f"[{name}] {k:8s} e32 = ({e32[k][0]:.3e}, {e32[k][1]:.3e})  kernel = ({e[0]:.3e}, {e[1]:.3e})  "
              f"ratio = ({e[0] / e32[k][0]:.2f}, {e[1] / e32[k][1]:.2f})")
        for i, metric in enumerate(("max", "l2")):
            if not e[i] <= TOL_FACTOR * e32[k][i]:
                bad.append((k, metric, e[i], e32[k][i]))
    assert not bad, f"{name}: beyond {TOL_FACTOR} x the fp32 statement's error: {bad}"
    mid = s64["median_id"]
    want = np.where(mid >= 0, geom_depths[np.maximum(mid, 0)], np.float32(0.0)).astype(np.float32)
    assert m["median"][keep].tobytes() == want[keep].tobytes(), \
        f"{name}: depth_median differs from the z of the statement's median Gaussian on {(m['median'] != want)[keep].sum()} kept pixels"
    # no exclusions
    assert ((m["median"] > 0) == (m["alpha"] >= 0.5)).all(), f"{name}: depth_median > 0 must hold exactly where alpha >= 0.5"
    empty = (s64["n_contrib"] == 0) & keep
    unlisted = np.repeat(np.repeat(s64["tile_len"] == 0, 16, axis=0), 16, axis=1)[:empty.shape[0], :empty.shape[1]]
    for k in MAPS:
        assert not m[k][empty | unlisted].any(), f"{name}: {k} is not exactly 0 on pixels without a contributor"


@pytest.mark.parametrize("name", CASES)
def test_maps_match_the_statement(backend, name):
    c = case(name)
    s64, e32, keep = oracle_of(name)
    m, _ = hip_maps(backend, c)
    assert (s64["n_contrib"] == 0).any() or name == "trained"
    check(name, m, s64, e32, keep, c["geom"]["depths"])


def test_two_calls_give_identical_bits(backend):
    c = case("ragged3000")
    r, _ = forward(backend, c)
    m1, m2 = maps_of(backend, r, c), maps_of(backend, r, c)
    for k in MAPS:
        assert m1[k].tobytes() == m2[k].tobytes(), k


def test_cull_levels_give_identical_bits(backend):
    c = case("ragged3000")
    base, _ = hip_maps(backend, c, cull=0)
    for cull in (1, 2):
        m, _ = hip_maps(backend, c, cull=cull)
        for k in MAPS:
            assert m[k].tobytes() == base[k].tobytes(), f"cull {cull}: {k}"


def test_any_subset_of_outputs(backend):
    c = case("small800")
    r, _ = forward(backend, c)
    full = maps_of(backend, r, c)
    for n in range(0, 3):
        for want in itertools.combinations(MAPS, n):
            m = maps_of(backend, r, c, want=want)
            assert set(m) == set(want)
            for k in want:
                assert m[k].tobytes() == full[k].tobytes(), f"want = {want}: {k}"
    with pytest.raises(ValueError, match="unknown"):
        r.depth_maps(c["W"], c["H"], want=("normal",))


def test_the_depth_pass_leaves_the_forward_state_alone(backend):
    """backward after depth_maps on the same state == backward of a fresh forward"""
    c = case("small800")
    d = backend.dev

    def backward(r, f):
        g = r.backward(d(c["w"]), f["xyz"], *f["common"], sh_degree=c["deg"], scale_modifier=c["mod"], want_conic=True, **f["dev"])
        backend.sync()
        return {k: (None if v is None else backend.host(v).copy()) for k, v in g.items()}

    r1, f1 = forward(backend, c)
    calls = r1.state_calls
    maps_of(backend, r1, c)
    assert r1.state_calls == calls, "depth_maps does not end the forward state"
    g1 = backward(r1, f1)
    r2, f2 = forward(backend, c)
    g2 = backward(r2, f2)
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None)
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k
    m_after = maps_of(backend, r1, c)      # and the maps after a backward are the maps
    m_fresh = maps_of(backend, r2, c)
    for k in MAPS:
        assert m_after[k].tobytes() == m_fresh[k].tobytes(), k


def test_error_conditions(backend):
    c = case("small800")
    W, H = c["W"], c["H"]
    like = backend.dev(np.zeros(1, np.float32))
    r = Rasterizer(0, lib=backend.lib)
    with pytest.raises(RuntimeError, match="no state"):
        r.depth_maps(W, H, like=like)
    with pytest.raises(RuntimeError, match="TILE_ROWS"):
        r2, _ = forward(backend, c, rows=2)
        r2.depth_maps(W, H, like=like)
    r, _ = forward(backend, c)
    with pytest.raises(RuntimeError, match="do not match"):
        r.depth_maps(W + 1, H, like=like)
    with pytest.raises(RuntimeError, match="do not match"):
        r.depth_maps(W, H - 1, like=like)
    r.reserve(4 * c["arrays"]["means3D"].shape[0], 2, W, H, 4_000_000)      # may reallocate what the pass reads
    with pytest.raises(RuntimeError, match="no state"):
        r.depth_maps(W, H, like=like)
    r, _ = forward(backend, c)
    r.set_option(_lib.OPT_PAIR_BATCH, 2)
    with pytest.raises(RuntimeError, match="PAIR_BATCH"):
        r.depth_maps(W, H, like=like)
    # a forward that overflowed its arena (far too small on purpose); its status has reached the host after a sync
    r = Rasterizer(0, lib=backend.lib)
    r.reserve(c["arrays"]["means3D"].shape[0], 1, W, H, 64)
    r, _ = forward(backend, c, r=r, sync=False)
    backend.sync()
    with pytest.raises(RuntimeError, match="overflowed"):
        r.depth_maps(W, H, like=like)
    r, _ = forward(backend, c, r=r)            # synchronous forward: grows the arena and repeats
    s64, e32, keep = oracle_of("small800")
    check("small800/after overflow", maps_of(backend, r, c), s64, e32, keep, c["geom"]["depths"])


def test_render_views_ends_the_forward_state(backend):
    from test_raster_parity import scene
    W, H, f = 96, 80, 90.0
    g, s, q, o, shs, left, right = scene(800, 5, W, H, f)
    c = case("small800")
    r, _ = forward(backend, c)
    from gs2mesh_amd.rasterizer import camera_from
    d = backend.dev
    gauss = dict(xyz=d(g["xyz"]), scaling=d(g["scaling"]), rotation=d(g["rotation"]), opacity=d(g["opacity"]),
                 features_dc=d(g["features_dc"]), features_rest=d(g["features_rest"]), raw=True, sh_degree=3)
    r.render_views(gauss, [camera_from(left)], bg=(0.1, 0.2, 0.3))
    with pytest.raises(RuntimeError, match="no state"):
        r.depth_maps(W, H, like=d(np.zeros(1, np.float32)))


def test_no_gaussians_gives_zero_maps(backend):
    c = case("small800")
    empty = dict(c, arrays={k: (None if v is None else v[:0]) for k, v in c["arrays"].items()})
    r, _ = forward(backend, empty)
    m = maps_of(backend, r, c)
    for k in MAPS:
        assert not m[k].any(), k
