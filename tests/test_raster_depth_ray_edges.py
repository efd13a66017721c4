"""The ray depth pass (gs2m_rasterize_depth_ray) at its edges, on both back-ends: images below a tile and one pixel over it, lists
whose ray records cross the 64-instance staging batches, the degenerate Gaussians of the definition (fronto-parallel discs,
rank <= 1, isotropic, edge-on), ids beyond 65536 and a listed Gaussian with an infinite scale.  The scenes are built with the blocks of tests/test_raster_backward_edges.py
(identity camera: world = view space).

Every case asserts its purpose on the fp64 statement (tests/ray_depth_statement.py) first.  Where the statement is the yardstick,
the bound is that of tests/test_raster_depth_ray.py: TOL_FACTOR x the fp32 statement's own error on the kept pixels plus
(8 + 2 sqrt(n)) 2^-24, n = the longest run of contributors, for ``expected`` and for ``median`` as a value.  Closed-form
expectations carry their own argument next to the assertion.

Non-finite input: NaN scales and NaN or infinite rotations make the 3D covariance NaN, the radius 0 and the rect empty, and the
record pass skips Gaussians without a rect: no walk can read such a record, and no case is built for them.  An INFINITE scale is
different: Sigma is +-inf without a NaN, and under a camera with a full view rotation, far enough off the axis, the forward lists
such a Gaussian on the whole grid with a NaN conic and alpha 0.99 on every pixel (under the identity camera a structural zero of
J meets the inf and it is not listed, which is all tests/test_raster_forward_edges.py shows).  Case 8 builds it.
"""
import functools

import numpy as np
import pytest
import torch

import depth_statement as ds
import ray_depth_statement as rds
from test_raster_backward import TOL_FACTOR
from test_raster_backward_edges import finish, place, random_shs, scales_px, scan_scenes, size_case, unit_quats
from test_raster_depth import MAPS, forward, maps_of
from test_raster_depth_edges import SIZE_SEEDS
from test_raster_depth_ray import ray_maps_of

U = 2.0 ** -24
IDENT = np.array([1, 0, 0, 0], np.float32)


def run(be, c):
    """-> (ray maps, centre maps) of one forward"""
    r, f = forward(be, c)
    return ray_maps_of(be, r, c, f), maps_of(be, r, c)


_STATEMENTS = {}


def statements(key, build):
    """-> (case, fp64 statement, fp32 statement, keep); one evaluation per case, shared between the back-ends"""
    if key not in _STATEMENTS:
        c = build()
        s64 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float64)
        s32 = rds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float32)
        keep = (c["w"][0] != 0) & ~s64["near05"] & ~s64["grazing"]
        for v in s64.values():
            v.setflags(write=False)
        _STATEMENTS[key] = (c, s64, s32, keep)
    return _STATEMENTS[key]


def check_against_statement(name, m, centre, s64, s32, keep, min_keep=0.9):
    assert keep.mean() >= min_keep, f"{name}: only {keep.mean():.1%} of the pixels are kept"
    np.testing.assert_array_equal(s32["median_id"][keep], s64["median_id"][keep])
    floor = (8 + 2 * np.sqrt(float(s64["n_contrib"].max()))) * U
    for k in ("expected", "median"):
        e32, e = ds.errors(s32[k], s64[k], keep), ds.errors(m[k], s64[k], keep)
        print(f"[{name}] {k:8s} e32 = ({e32[0]:.3e}, {e32[1]:.3e})  kernel = ({e[0]:.3e}, {e[1]:.3e})")
        for i in range(2):
            assert e[i] <= TOL_FACTOR * e32[i] + floor, (name, k, ("max", "l2")[i], e[i], e32[i])
    assert m["alpha"].tobytes() == centre["alpha"].tobytes(), name
    assert ((m["median"] > 0) == (m["alpha"] >= 0.5)).all(), name
    empty = (s64["n_contrib"] == 0) & keep
    for k in MAPS:
        assert not m[k][empty].any(), f"{name}: {k} on pixels without a contributor"


def assert_centre_bits(name, m, centre):
    for k in MAPS:
        assert m[k].tobytes() == centre[k].tobytes(), f"{name}: {k} differs from the centre map"


# ---- 1: image sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sorted(SIZE_SEEDS))
def test_images_below_a_tile_and_one_pixel_over(backend, W, H):
    c, s64, s32, keep = statements(f"size{W}x{H}", functools.partial(size_case, W, H, SIZE_SEEDS[W, H]))
    assert s64["tile_len"].shape == (1, (W + 15) // 16) and s64["tile_len"].min() > 0
    assert (s64["n_contrib"] > 0).all(), "Gaussian 0 covers every pixel"
    m, centre = run(backend, c)
    check_against_statement(f"size{W}x{H}", m, centre, s64, s32, keep)
    assert np.abs(m["expected"] - centre["expected"]).max() > 1e-3, "the ray depth is not the centre's"


# ---- 2: lists whose records cross the staging batches -------------------------------------------------------------------------
STACK_O, STACK_Z = 0.02, 2.5


def stack_case(n):
    """one 16 x 16 tile, n flat discs (in-plane sigma 9 px, thickness 1e-4, opacity 0.02) centred ON pixel (8, 8) at one depth,
    disc i tilted about y by 15 + 45 i / (n - 1) degrees and about x by +-10: the list is their id order, every instance has a
    record of its own, and a record staged into the wrong slot of a batch moves the depth of every pixel off the centre column"""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(911)
    xyz = np.repeat(place([8.0], [8.0], [STACK_Z], W, H, f), n, axis=0)
    s = np.tile(np.array([9.0 * STACK_Z / f, 9.0 * STACK_Z / f, 1e-4]), (n, 1))
    ty = np.radians(15.0 + 45.0 * np.arange(n) / (n - 1))
    tx = np.radians(10.0) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    # q = q_y(ty) q_x(tx)
    q = np.stack([np.cos(ty / 2) * np.cos(tx / 2), np.cos(ty / 2) * np.sin(tx / 2), np.sin(ty / 2) * np.cos(tx / 2),
                  -np.sin(ty / 2) * np.sin(tx / 2)], axis=1)
    return finish(f"ray_stack{n}", xyz, s, q, np.full(n, STACK_O), random_shs(rng, n), W, H, f)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_tilted_stack_crosses_the_batch_boundaries(backend, n):
    c, s64, s32, keep = statements(f"ray_stack{n}", functools.partial(stack_case, n))
    assert s64["tile_len"].tolist() == [[n]] and s64["n_contrib"].max() == n, "the centre pixel meets all n"
    assert not s64["grazing"].any()
    m, centre = run(backend, c)
    check_against_statement(f"ray_stack{n}", m, centre, s64, s32, keep)
    # every disc passes through the centre of pixel (8, 8): there the ray depth is the centre's z, but for the rounding of the
    # records (|w|, |c| and the quotient: a few 2^-24) and of the n-term mean
    assert abs(m["expected"][8, 8] / np.float32(STACK_Z) - 1) <= 2 * (n + 8) * U
    # off the centre column the tilt shows: 7 px at 20 px focal, tan 15..60 degrees
    assert np.abs(m["expected"][8, 1] - STACK_Z) > 0.1 and np.abs(s64["expected"][8, 1] - STACK_Z) > 0.1


# ---- 3: fronto-parallel discs ----------------------------------------------------------------------------------------------
def fronto_case(third):
    """40 x 24, a jittered grid of 15 x 9 discs at view depths 2..4 with the identity quaternion and scales (sx, sy, third)"""
    W, H, f = 40, 24, 35.0
    rng = np.random.default_rng(912)
    u, v = np.meshgrid(np.linspace(0, W - 1, 15), np.linspace(0, H - 1, 9))
    u, v = u.reshape(-1) + rng.uniform(-0.7, 0.7, u.size), v.reshape(-1) + rng.uniform(-0.7, 0.7, u.size)
    n = u.size
    z = rng.uniform(2.0, 4.0, n)
    s = scales_px(rng, rng.uniform(2.5, 4.0, n), z, f)
    s[:, 2] = third
    return finish(f"fronto{third}", place(u, v, z, W, H, f), s, np.tile(IDENT, (n, 1)), rng.uniform(0.3, 0.9, n),
                  random_shs(rng, n), W, H, f)


def test_fronto_parallel_discs_have_the_centre_bits(backend):
    """identity quaternion, identity camera, scales (sx, sy, 0): M = I exactly, sz = sqrt(0) = 0, lo = hi = z_c -- whatever t is"""
    c, s64, s32, keep = statements("fronto0", functools.partial(fronto_case, 0.0))
    c64 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float64)
    assert (s64["n_contrib"] > 0).mean() > 0.9 and (s64["median_id"] >= 0).mean() > 0.2
    assert np.array_equal(s64["expected"], c64["expected"]) and np.array_equal(s64["median"], c64["median"]), \
        "the statement's ray maps ARE its centre maps"
    lo, hi = rds.record_limits(c["arrays"], c["cam"])
    assert np.array_equal(lo, hi)
    m, centre = run(backend, c)
    assert_centre_bits("fronto0", m, centre)


# ---- 4: rank <= 1 ----------------------------------------------------------------------------------------------------------
def rank1_case():
    """32 x 16: 40 needles (s, 0, 0) with random rotations and 40 points (0, 0, 0), centred ON pixel centres (visible through
    the 0.3 px dilation alone, or along the needle), opacity 0.6..0.95, depths 2..4"""
    W, H, f = 32, 16, 30.0
    rng = np.random.default_rng(913)
    n = 80
    u, v = rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64)
    z = rng.uniform(2.0, 4.0, n)
    s = np.zeros((n, 3))
    s[:40, 0] = rng.uniform(2.0, 5.0, 40) * z[:40] / f
    return finish("rank1", place(u, v, z, W, H, f), s, unit_quats(rng, n), rng.uniform(0.6, 0.95, n), random_shs(rng, n), W, H, f)


def test_rank_one_and_zero_have_the_centre_bits(backend):
    """g = (s1 s2, s0 s2, s0 s1) = 0: no orientation, w = c = 0, den = 0, t = z_c, and z_c lies in [lo, hi]"""
    c, s64, s32, keep = statements("rank1", rank1_case)
    c64 = ds.depth_maps(c["arrays"], c["cam"], c["W"], c["H"], 1.0, torch.float64)
    med = np.unique(s64["median_id"][s64["median_id"] >= 0])
    assert (med < 40).any() and (med >= 40).any(), "a needle and a point are some pixel's median"
    assert np.array_equal(s64["expected"], c64["expected"]) and np.array_equal(s64["median"], c64["median"])
    m, centre = run(backend, c)
    assert_centre_bits("rank1", m, centre)


# ---- 5: one isotropic Gaussian -----------------------------------------------------------------------------------------------
def isotropic_case():
    """48 x 32, one isotropic Gaussian (sigma 6 px, opacity 0.9, a random rotation) off the axis, at pixel (37.3, 7.6), z = 2.5"""
    W, H, f = 48, 32, 40.0
    rng = np.random.default_rng(914)
    s = np.full((1, 3), np.float32(6.0 * 2.5 / f))
    return finish("isotropic", place([37.3], [7.6], [2.5], W, H, f), s, unit_quats(rng, 1), [0.9], random_shs(rng, 1), W, H, f)


def test_isotropic_gaussian_gives_the_nearest_point_of_the_ray(backend):
    """B = s^4 M M^T = s^4 I: t* = (mu . r) / (r . r).  In fp32: M M^T = I + E with |E| of a few 2^-24 (the quaternion's
    norm, R's entries); mu = t0 r + d with d perpendicular to r and |d| / |mu| < 0.3 within the Gaussian, so the relative error
    of t* from E is |E| |d| / |mu| < 2^-24, and the dot products and the quotient round about five times more: 8 x 2^-24"""
    c, s64, s32, keep = statements("isotropic", isotropic_case)
    cam, W, H = c["cam"], c["W"], c["H"]
    mu = c["arrays"]["means3D"][0].astype(np.float64)
    rx = ((2 * np.arange(W) + 1) / W - 1) * cam.tanfovx
    ry = ((2 * np.arange(H) + 1) / H - 1) * cam.tanfovy
    RX, RY = np.meshgrid(rx, ry)
    want = (mu[0] * RX + mu[1] * RY + mu[2]) / (RX * RX + RY * RY + 1)
    lo, hi = rds.record_limits(c["arrays"], cam)
    has = s64["median_id"] >= 0
    inside = has & (want > lo[0]) & (want < hi[0])
    # the statement takes the fp32 quaternion as given: its norm is 1 to a few 2^-24, and so is M M^T
    assert inside.sum() >= 50 and np.abs(s64["median"][inside] / want[inside] - 1).max() < 0.5 * U
    assert np.abs(want[inside] - mu[2]).max() > 0.02, "the nearest point of the ray is not at the centre's depth"
    m, centre = run(backend, c)
    check_against_statement("isotropic", m, centre, s64, s32, keep)
    got = m["median"][inside & ~s64["near05"]].astype(np.float64)
    assert np.abs(got / want[inside & ~s64["near05"]] - 1).max() <= 8 * U


# ---- 6: an edge-on disc ------------------------------------------------------------------------------------------------------
EDGE_Z = 3.0


def edge_on_case():
    """32 x 32: Gaussian 0 is a disc (in-plane sigma 0.6 world units, thickness 0, opacity 0.99) whose normal is the x axis,
    centred on the optical axis at z = 3: its plane contains the axis, it is seen through the 0.3 px dilation alone as a column of
    half a pixel sigma, and the rays of the two middle columns meet its plane at t = 0: clamped to lo = max(3 - 2.4, 0.2).
    Behind it a fronto-parallel slab at z = 5 covers the image."""
    W = H = 32
    f = 40.0
    rng = np.random.default_rng(915)
    xyz = np.array([[0.0, 0.0, EDGE_Z], [0.0, 0.0, 5.0]])
    s = np.array([[0.6, 0.6, 0.0], [8.0, 8.0, 0.0]])
    q = np.array([[np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0], IDENT])     # R_y(90 deg): local z -> x
    return finish("edge_on", xyz, s, q, [0.99, 0.7], random_shs(rng, 2), W, H, f)


def test_edge_on_disc_stays_inside_its_limits(backend):
    c, s64, s32, keep = statements("edge_on", edge_on_case)
    lo, hi = rds.record_limits(c["arrays"], c["cam"])
    assert abs(lo[0] - (EDGE_Z - 2.4)) < 1e-6 and abs(hi[0] - (EDGE_Z + 2.4)) < 1e-6 and lo[1] == hi[1] == 5.0
    first = s64["median_id"] == 0
    assert s64["grazing"][first].all() and first.sum() >= 16, "the disc is the median of its column, and grazing there"
    assert s64["grazing"].mean() > 0.05 and (s64["n_contrib"] > 0).all()
    m, centre = run(backend, c)
    check_against_statement("edge_on", m, centre, s64, s32, keep, min_keep=0.5)
    # the excluded pixels: finite (ray_maps_of) and in range -- the median inside the limits of its Gaussian, the mean
    # inside the limits of the two contributors (one rounding per term)
    slack = 1 + 8 * U
    decided = ~s64["near05"] & (c["w"][0] != 0)
    for j in (0, 1):
        sel = decided & (s64["median_id"] == j)
        assert (m["median"][sel] >= np.float32(lo[j]) / slack).all() and (m["median"][sel] <= np.float32(hi[j]) * slack).all(), j
    assert (m["expected"] >= lo.min() / slack).all() and (m["expected"] <= hi.max() * slack).all()
    assert (m["median"][first & decided] < EDGE_Z - 2.0).any(), "the clamp at lo binds in the disc's column"


# ---- 7: ids beyond 65536 ------------------------------------------------------------------------------------------------------
def test_ids_beyond_65536(backend):
    """the scan scene of the backward's edge tests: 2 x 65536 + 700 Gaussians, all behind the camera but 301 with ids up to
    131 700; the compact scene holds the visible ones in the same order, so the lists are the same up to relabelling and the ray
    records are indexed by the large ids"""
    big, compact, ids = scan_scenes()
    assert big["arrays"]["means3D"].shape[0] > 2 * 65536 and ids.max() >= 131072
    c, s64, s32, keep = statements("scan", lambda: compact)
    far = ids[np.unique(s64["median_id"][s64["median_id"] >= 0])]
    assert (far >= 65536).any(), "a Gaussian with an id beyond 65536 is some pixel's median"
    (m_big, _), (m_cmp, centre) = run(backend, big), run(backend, compact)
    for k in MAPS:
        assert m_big[k].tobytes() == m_cmp[k].tobytes(), k
    check_against_statement("scan", m_cmp, centre, s64, s32, keep)


def test_everything_culled_gives_zero_maps(backend):
    from test_raster_backward_edges import case as edge_case
    c = edge_case("culled")
    m, _ = run(backend, c)
    for k in MAPS:
        assert not m[k].any(), k


# ---- 8: an infinite scale ------------------------------------------------------------------------------------------------------
INF_SEED, INF_Z = 52, 2.0


def infinite_scale_case(seed=INF_SEED):
    """64 x 64, focal 32 (tan fov = 1), a camera with a generic pose (posed_case).  Gaussian 0 has scales (0.1, inf, 0.1), a
    generic rotation, opacity 0.7, and sits in FRONT of everything at view depth 2, near the image corner (tx / tz, ty / tz
    about 0.85).  computeCov3D gives it a Sigma of +-inf without a NaN; computeCov2D -- whose J has no structural zero to meet an
    inf once W is full, and whose two rows are far from orthogonal that far off the axis -- can then give a = c = +inf and
    b = +-inf: det = NaN passes ``det == 0``, the radius saturates at INT_MAX and the rect is the whole grid.  Whether it does
    depends on the signs of T's rows against the infinite axis: the seed is one for which it does, and the test asserts that
    first.  The conic is NaN, so power is NaN, neither skip decision fires, alpha = min(0.99, NaN) = 0.99 on EVERY pixel.
    Behind it, at view depths 3..4, 40 tilted flat discs."""
    from test_raster_depth_ray import posed_case
    W = H = 64
    f = 32.0
    rng = np.random.default_rng(916)
    n = 40
    z = np.concatenate([[INF_Z], rng.uniform(3.0, 4.0, n)])
    u = np.concatenate([[59.0], rng.uniform(0, W - 1, n)])
    v = np.concatenate([[60.0], rng.uniform(0, H - 1, n)])
    s = np.concatenate([[[0.1, np.inf, 0.1]], np.tile([0.6, 0.6, 1e-4], (n, 1))])
    th = np.radians(rng.uniform(-50.0, 50.0, n))
    q = np.concatenate([unit_quats(np.random.default_rng(seed), 1).astype(np.float64),
                        np.stack([np.cos(th / 2), 0 * th, np.sin(th / 2), 0 * th], axis=1)])
    o = np.concatenate([[0.7], rng.uniform(0.5, 0.9, n)])
    return posed_case("infinite_scale", place(u, v, z, W, H, f), s, q, o, random_shs(rng, n + 1), W, H, f, seed=seed)


def test_infinite_scale_contributes_a_finite_depth(backend):
    """a LISTED Gaussian with an infinite scale: g holds an inf, so gmax is not finite and w = c = 0 (t = z_c); sz = inf, so
    lo = max(z_c - inf, 0.2) = 0.2 and hi = inf.  Its contribution is z_c, finite and in [0.2, inf), at weight 0.99 on every
    pixel.  (NaN scales and NaN or infinite rotations make Sigma NaN: a NaN conic's determinant chain ends in radius 0, such a
    Gaussian is never listed.  The fmaxf rule of sz -- a NaN sum counts as 0 -- needs 0 x inf in M[2][k] s_k, an exact zero of
    the view rotation: under such a camera the same zero meets the inf in computeCov2D and the Gaussian is not listed either.)"""
    c = infinite_scale_case()
    g, W, H = c["geom"], c["W"], c["H"]
    assert g["radii"][0] == 2 ** 31 - 1 and g["rect"][0].tolist() == [0, 0, W // 16, H // 16], "the forward lists it, on every tile"
    assert np.isnan(g["conic_opacity"][0][:3]).all() and np.isfinite(g["depths"]).all()
    z0 = g["depths"][0]
    assert abs(float(z0) - INF_Z) < 1e-5 and (g["depths"][1:] > 2.9).all() and (g["radii"][1:] > 0).all()
    zc = torch.tensor(g["depths"].astype(np.float64))
    w, cc, lo, hi = rds.records(c["arrays"], c["cam"], 1.0, torch.float64, zc)
    assert not w[0].any() and not cc[0].any() and lo[0] == 0.2 and hi[0] == float("inf"), "the record the contract spells out"
    assert w[1:].abs().amax(dim=(1, 2)).min() > 0.5 and torch.isfinite(hi[1:]).all()
    m, centre = run(backend, c)             # every map finite: ray_maps_of / maps_of
    cap = np.float32(0.99)
    assert (m["alpha"] >= cap).all() and m["alpha"].tobytes() == centre["alpha"].tobytes()
    # T = 0.01 behind the first instance: it is every pixel's median, with its z_c to the bit
    assert (m["median"] == z0).all() and (centre["median"] == z0).all()
    # expected = (0.99 z0 + sum w_j z_j(p)) / (0.99 + sum w_j), sum w_j <= 0.01 and every z_j(p) within the limits of its disc
    far = float(hi[1:].max())
    assert (m["expected"] >= np.float32(0.2)).all()
    assert np.abs(m["expected"].astype(np.float64) - float(z0)).max() <= (0.01 / 0.99) * (far - 0.2) + 1e-5
    assert np.abs(m["expected"] - centre["expected"]).max() > 1e-4, "the discs behind it still get their ray depth"
