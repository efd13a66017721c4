"""The depth pass (gs2m_rasterize_depth, k_blend_depth) at its edges, on both back-ends: images below a tile and one pixel over
it, lists that end at the 64-instance staging batches, a plane at one view depth, saturation (stop BEFORE accumulating), the 0.99
cap, a median that falls on the second of two layers, and ids beyond 65536.  The scenes are built with the blocks of
tests/test_raster_backward_edges.py (identity camera: world = view space, so a Gaussian placed at z has view depth z exactly).

Every case asserts its purpose on the fp64 statement (tests/depth_statement.py) first.  Where the statement is the yardstick,
the bound is that of tests/test_raster_depth.py -- TOL_FACTOR x the fp32 statement's own error on the kept pixels -- plus a
floor of (8 + 2 sqrt(n)) x 2^-24, n = the longest run of contributors of the case.  On a few hundred designed pixels the fp32
statement can be exact to the last bit where the kernel's fast exp and FMA order are one rounding away (the 8: one rounding
of alpha = 1 - T is 2^-24 of the map's maximum), and the statement sums a pixel's n terms with torch's pairwise sum
(error ~ log2 n roundings) where the kernel adds them front to back (~ sqrt n roundings, at most n): with n = 129 equal
terms the statement's own error says nothing about a sequential sum.  Closed-form expectations carry their own rounding
argument next to the assertion.
"""
import functools

import numpy as np
import pytest
import torch

import depth_statement as ds
from test_raster_backward import TOL_FACTOR
from test_raster_backward_edges import finish, place, random_shs, scales_px, scan_scenes, size_case, unit_quats
from test_raster_depth import MAPS, forward, maps_of

U = 2.0 ** -24


def run(be, c):
    r, _ = forward(be, c)
    return maps_of(be, r, c)


_STATEMENTS = {}


def statements(key, build):
    """-> (case, fp64 statement, fp32 statement, keep); one evaluation per case, shared between the back-ends"""
    if key not in _STATEMENTS:
        _STATEMENTS[key] = _evaluate(build())
    return _STATEMENTS[key]


def _evaluate(c):
    s64 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float64)
    s32 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float32)
    keep = (c["w"][0] != 0) & ~s64["near05"]
    for v in s64.values():
        v.setflags(write=False)
    return c, s64, s32, keep


def check_against_statement(name, m, c, s64, s32, keep):
    assert keep.mean() >= 0.95, f"{name}: only {keep.mean():.1%} of the pixels are kept"
    np.testing.assert_array_equal(s32["median_id"][keep], s64["median_id"][keep])
    floor = (8 + 2 * np.sqrt(float(s64["n_contrib"].max()))) * U
    for k in ("alpha", "expected"):
        e32, e = ds.errors(s32[k], s64[k], keep), ds.errors(m[k], s64[k], keep)
        print(f"[{name}] {k:8s} e32 = ({e32[0]:.3e}, {e32[1]:.3e})  kernel = ({e[0]:.3e}, {e[1]:.3e})")
        for i in range(2):
            assert e[i] <= TOL_FACTOR * e32[i] + floor, (name, k, ("max", "l2")[i], e[i], e32[i])
    mid = s64["median_id"]
    want = np.where(mid >= 0, c["geom"]["depths"][np.maximum(mid, 0)], np.float32(0.0)).astype(np.float32)
    assert m["median"][keep].tobytes() == want[keep].tobytes(), name
    assert ((m["median"] > 0) == (m["alpha"] >= 0.5)).all(), name
    empty = (s64["n_contrib"] == 0) & keep
    for k in MAPS:
        assert not m[k][empty].any(), f"{name}: {k} on pixels without a contributor"


# ---- 1: image sizes ---------------------------------------------------------------------------------------------------------
# seeds of size_case with which no pixel of the image sits on a threshold (one excluded pixel of 5 x 3 is 7 % of the image)
SIZE_SEEDS = {(5, 3): 413, (17, 16): 410}


@pytest.mark.parametrize("W,H", sorted(SIZE_SEEDS))
def test_images_below_a_tile_and_one_pixel_over(backend, W, H):
    c, s64, s32, keep = statements(f"size{W}x{H}", functools.partial(size_case, W, H, SIZE_SEEDS[W, H]))
    assert s64["tile_len"].shape == (1, (W + 15) // 16) and s64["tile_len"].min() > 0
    assert (s64["n_contrib"] > 0).all(), "Gaussian 0 covers every pixel"
    m = run(backend, c)
    check_against_statement(f"size{W}x{H}", m, c, s64, s32, keep)


# ---- 2: lists that end at the staging batches -------------------------------------------------------------------------------
STACK_O, STACK_Z = 0.02, 2.5


def stack_case(n):
    """one 16 x 16 tile, n identical Gaussians (sigma 9 px, opacity 0.02, centred ON pixel (8, 8)) at one depth: the list is
    their id order, (1 - 0.02)^129 = 0.074 so nothing saturates, and T passes 0.5 at the 35th"""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(901)
    xyz = np.repeat(place([8.0], [8.0], [STACK_Z], W, H, f), n, axis=0)
    s = np.repeat(scales_px(rng, [9.0], [STACK_Z], f, aniso=0.0), n, axis=0)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    return finish(f"stack{n}", xyz, s, q, np.full(n, STACK_O), random_shs(rng, n), W, H, f)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_coincident_stack_ends_at_the_batch_boundaries(backend, n):
    c, s64, s32, keep = statements(f"stack{n}", functools.partial(stack_case, n))
    assert s64["tile_len"].tolist() == [[n]] and s64["n_contrib"].max() == n, "every pixel near the centre meets all n"
    z = np.float32(STACK_Z)
    assert (c["geom"]["depths"] == z).all()
    m = run(backend, c)
    check_against_statement(f"stack{n}", m, c, s64, s32, keep)
    # all contributors share one z: the median IS z, and expected = (sum w z) / (sum w) is z but for one rounding per term
    has = m["alpha"] >= 0.5
    assert has[8, 8] == (1 - (1 - STACK_O) ** n >= 0.5)
    assert (m["median"][has] == z).all() and not m["median"][~has].any()
    hit = m["alpha"] > 0
    assert np.abs(m["expected"][hit] / z - 1).max() <= 2 * (n + 2) * U
    # at the centre G = 1 up to the rounding of the projected mean (|d| < 1e-5 px, sigma 9 px: 1 - G < 1e-12), so every
    # instance has alpha = 0.02f and T = (1 - 0.02f)^n with one rounding per factor: the count n shows in alpha itself
    want = 1 - (1 - float(np.float32(STACK_O))) ** n
    assert abs(m["alpha"][8, 8] - want) <= (n + 2) * U, (m["alpha"][8, 8], want)
    assert abs(want - (1 - (1 - float(np.float32(STACK_O))) ** (n - 1))) > 100 * (n + 2) * U, "n - 1 instances would be told apart"


# ---- 3: a plane at one view depth ---------------------------------------------------------------------------------------------
PLANE_D = 3.25


def plane_case():
    """40 x 24, a jittered grid of 15 x 9 Gaussians (sigma 2.5..4 px, opacity 0.3..0.9), all at view depth 3.25"""
    W, H, f = 40, 24, 35.0
    rng = np.random.default_rng(902)
    u, v = np.meshgrid(np.linspace(0, W - 1, 15), np.linspace(0, H - 1, 9))
    u, v = u.reshape(-1) + rng.uniform(-0.7, 0.7, u.size), v.reshape(-1) + rng.uniform(-0.7, 0.7, u.size)
    n = u.size
    z = np.full(n, PLANE_D)
    return finish("plane", place(u, v, z, W, H, f), scales_px(rng, rng.uniform(2.5, 4.0, n), z, f), unit_quats(rng, n),
                  rng.uniform(0.3, 0.9, n), random_shs(rng, n), W, H, f)


def test_plane_at_one_depth(backend):
    c, s64, s32, keep = statements("plane", plane_case)
    d = np.float32(PLANE_D)
    assert (c["geom"]["depths"] == d).all(), "identity camera: the view depth is the placed z, exactly"
    n = int(s64["n_contrib"].max())
    has64 = s64["median_id"] >= 0
    assert (s64["n_contrib"] > 0).all() and 0.2 < has64.mean() and n >= 8
    m = run(backend, c)
    check_against_statement("plane", m, c, s64, s32, keep)
    # S and Z are sums of at most n terms w and w d, rounded once per term (and once more per product without FMA); their
    # quotient rounds once: |expected / d - 1| <= 2 (n + 2) 2^-24
    assert np.abs(m["expected"] / d - 1).max() <= 2 * (n + 2) * U
    has = m["alpha"] >= 0.5
    assert (m["median"][has] == d).all() and not m["median"][~has].any()


# ---- 4: saturation --------------------------------------------------------------------------------------------------------
SAT_FAR = 1000.0


def saturation_case():
    """one 16 x 16 tile: three slabs (sigma 200 px: G > 0.997 on the tile) at opacity 0.95 and z = 2.00, 2.01, 2.02 leave
    T in 1.25e-4 .. 1.5e-4; a fourth at opacity 0.95 and z = 1000 would take it to 7e-6 < 1e-4: the pixel stops BEFORE
    accumulating it.  Accumulated, its weight 0.95 x 1.25e-4 x 1000 would move the expected depth from 2.0 to 2.1."""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(903)
    z = np.array([2.0, 2.01, 2.02, SAT_FAR])
    return finish("saturation", place([7.5] * 4, [7.5] * 4, z, W, H, f), scales_px(rng, [200.0] * 4, z, f, aniso=0.0),
                  np.tile(np.array([1, 0, 0, 0], np.float32), (4, 1)), np.full(4, 0.95), random_shs(rng, 4), W, H, f)


def test_the_saturating_instance_is_not_accumulated(backend):
    c, s64, s32, keep = statements("saturation", saturation_case)
    assert s64["tile_len"].tolist() == [[4]] and (s64["n_contrib"] == 3).all(), "the far slab is listed and never contributes"
    assert keep.all()
    m = run(backend, c)
    check_against_statement("saturation", m, c, s64, s32, keep)
    assert m["expected"].max() < 2.02 and m["expected"].min() > 2.0, "the far z must not appear"
    assert (m["median"] == np.float32(2.0)).all()            # 1 - 0.95 G <= 0.5 after the first slab
    assert (m["alpha"] < 1 - 1.0e-4).all() and (m["alpha"] > 1 - 1.6e-4).all(), "T stays at the three slabs' product"


# ---- 5: the cap ---------------------------------------------------------------------------------------------------------------
def cap_case():
    """one 16 x 16 tile, one Gaussian of opacity 1 (sigma 30 px, centred ON pixel (8, 8)): o G > 0.99 within 4 px of the centre"""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(904)
    return finish("cap", place([8.0], [8.0], [2.0], W, H, f), scales_px(rng, [30.0], [2.0], f, aniso=0.0),
                  np.array([[1, 0, 0, 0]], np.float32), [1.0], random_shs(rng, 1), W, H, f)


def test_the_cap_binds(backend):
    c, s64, s32, keep = statements("cap", cap_case)
    capped64 = s64["alpha"] >= 0.99 - 1e-12
    assert 20 <= capped64.sum() < 200, "the cap binds near the centre only"
    m = run(backend, c)
    check_against_statement("cap", m, c, s64, s32, keep)
    # T = 1 - 0.99f and alpha = 1 - T are both exact (Sterbenz): the capped pixels hold 0.99f to the bit, none holds more
    cap = np.float32(0.99)
    assert m["alpha"].max() == cap and m["alpha"][8, 8] == cap
    assert ((m["alpha"] == cap) & keep).sum() >= (capped64 & keep).sum() - 4
    assert (m["median"] == np.float32(2.0)).all() and (m["expected"] == np.float32(2.0)).all()    # one contributor: Z / S = z


# ---- 6: the median on the second layer ----------------------------------------------------------------------------------------
def two_layer_case():
    """one 16 x 16 tile, two slabs (sigma 200 px) of opacity 0.4 at z = 2 and z = 3: T = 0.6 after the first (no median yet),
    0.36 after the second"""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(905)
    z = np.array([2.0, 3.0])
    return finish("two_layers", place([7.5] * 2, [7.5] * 2, z, W, H, f), scales_px(rng, [200.0] * 2, z, f, aniso=0.0),
                  np.tile(np.array([1, 0, 0, 0], np.float32), (2, 1)), np.full(2, 0.4), random_shs(rng, 2), W, H, f)


def test_the_median_falls_on_the_second_layer(backend):
    c, s64, s32, keep = statements("two_layers", two_layer_case)
    assert (s64["median_id"] == 1).all() and (s64["n_contrib"] == 2).all() and keep.all()
    m = run(backend, c)
    check_against_statement("two_layers", m, c, s64, s32, keep)
    assert (m["median"] == np.float32(3.0)).all()
    # (0.4 x 2 + 0.24 x 3) / 0.64 = 2.375 at G = 1; G > 0.997 on the tile moves the weights by under 0.3 %
    assert np.abs(m["expected"] - 2.375).max() < 2e-3


# ---- 7: ids beyond 65536 ------------------------------------------------------------------------------------------------------
def test_ids_beyond_65536(backend):
    """the scan scene of the backward's edge tests: 2 x 65536 + 700 Gaussians, all behind the camera but 301 with ids up to
    131 700; the compact scene holds the visible ones in the same order, so the lists are the same up to relabelling"""
    big, compact, ids = scan_scenes()
    assert big["arrays"]["means3D"].shape[0] > 2 * 65536 and ids.max() >= 131072
    s64 = ds.depth_maps(compact["arrays"], compact["cam"], compact["W"], compact["H"], 1.0, torch.float64)
    far = ids[np.unique(s64["median_id"][s64["median_id"] >= 0])]
    assert (far >= 65536).any(), "a Gaussian with an id beyond 65536 is some pixel's median"
    m_big, m_cmp = run(backend, big), run(backend, compact)
    for k in MAPS:
        assert m_big[k].tobytes() == m_cmp[k].tobytes(), k
    s32 = ds.depth_maps(compact["arrays"], compact["cam"], compact["W"], compact["H"], 1.0, torch.float32)
    keep = (compact["w"][0] != 0) & ~s64["near05"]
    check_against_statement("scan", m_cmp, compact, s64, s32, keep)


def test_everything_culled_gives_zero_maps(backend):
    from test_raster_backward_edges import case as edge_case
    c = edge_case("culled")
    m = run(backend, c)
    for k in MAPS:
        assert not m[k].any(), k
