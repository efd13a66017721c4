"""Gradients through the depth and opacity maps (gs2m_rasterize_backward_depth) at their edges, on both back-ends: images below
a tile and partial tiles (13 x 9, 17 x 16), tile lists of exactly 63 / 64 / 65 / 129 instances with the median at the last
instance of one 64-instance batch and at the first of the next, the median in an earlier batch than the last contributor,
saturating pixels, pixels without a median, a single-contributor pixel, the 0.99 cap, an empty tile, Gaussians over more than
one tile (row value nine summed over slots).  EVERY scene is seen by a tilted camera: vm[2], vm[6] and vm[10] are all non-zero,
so dL/dz reaches all three components of dL/dmean3D.

Every scene is built for one purpose and that purpose is asserted on the fp64 statement (tests/depth_grad_statement.py) first.
A statement result is computed once per case, shared between the back-ends and never modified.

Loss and weights as in tests/test_raster_depth_backward.py (all four terms, seeded, zero on threshold pixels and, for the median,
where a T sits at 0.5; at most 1 % of the pixels).  Bar, as in tests/test_raster_backward_edges.py: per Gaussian,
e_i = max_j |g[i,j] - g64[i,j]| / max(n_i, PHI S) with n_i = max_j |g64[i,j]|, S = max_i n_i, PHI = 1e-3, at most TOL_FACTOR = 4 x
the same metric of the SAME statement in fp32; the per-tensor check of test_raster_backward is applied too.  An entry whose
sum is ill-conditioned is judged, that entry alone, by the worst of several fp32 evaluations of the statement (``judge``).

A saturated pixel always has a median: the walk stops when T (1 - alpha) < 1e-4 with alpha <= 0.99, i.e. at T < 0.01, long after
T passed 0.5.  So "saturation without a median" cannot occur; the saturation scene asserts both kinds that can: pixels whose
median is the last contributor before the stop, and pixels whose median lies earlier.
"""
import functools

import numpy as np
import pytest
import torch

import depth_grad_statement as dgs
import depth_statement
import oracle
from gs2mesh_amd import synthetic
from test_raster_backward import TOL_FACTOR, errors
from test_raster_backward_edges import BG, E32_CEILING, ORDERS, PHI, per_gaussian, place, random_shs, scales_px, unit_quats
from test_raster_depth_backward import hip_grads


def tilted_camera(W, H, f):
    """rotated about x and y and shifted: every entry of the view matrix's z row is non-zero"""
    ax, ay = 0.35, -0.45
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    R, t = Rx @ Ry, np.array([0.3, -0.2, 0.5])
    cam = synthetic.stereo_cameras(np.concatenate([R, t[:, None]], axis=1), W, H, f, f, 0.245)[0]
    vm = np.asarray(cam.world_view_transform, np.float64).reshape(16)
    assert min(abs(vm[2]), abs(vm[6]), abs(vm[10])) > 0.1
    return cam, R, t


def finish(name, xyz_view, s, q, o, shs, W, H, f, seed=77):
    """xyz_view: centres in VIEW space (test_raster_backward_edges.place).  -> the case dict of test_raster_backward.case plus
    the four seeded weight maps ``weights`` (threshold pixels zeroed; the median's near05 mask is applied by oracle_of)"""
    cam, R, t = tilted_camera(W, H, f)
    xyz = ((np.asarray(xyz_view, np.float64) - t) @ R).astype(np.float32)       # world = R^T (view - t)
    s, q, shs = (np.ascontiguousarray(a, np.float32) for a in (s, q, shs))
    o = np.ascontiguousarray(o, np.float32).reshape(-1)
    arrays = dict(means3D=xyz, opacities=o, shs=shs, colors_precomp=None, scales=s, rotations=q, cov3D_precomp=None)
    geom = oracle.preprocess(xyz, s, q, o, shs, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, W, H,
                             cam.tanfovx, cam.tanfovy, sh_degree=3)
    pl, ranges = oracle.bin_instances(geom, W, H)
    fb = oracle.render_flip_bounds(W, H, ranges, pl, geom["means2D"], geom["conic_opacity"], 1.0, rel_eps=1e-4)
    near = (fb["n_alpha"].astype(np.int64) + fb["n_T"] + fb["n_power"]) > 0
    rng = np.random.default_rng(seed)
    w = dict(wC=rng.uniform(-1.0, 1.0, (3, H, W)).astype(np.float32))
    w.update({k: rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32) for k in ("wD", "wM", "wA")})
    for v in w.values():
        v[..., near] = 0.0
    return dict(name=name, arrays=arrays, cam=cam, W=W, H=H, bg=BG, deg=3, mod=1.0, weights=w, near=near, geom=geom)


# ---- the scenes ---------------------------------------------------------------------------------------------------------
def size_case(W, H):
    """40 Gaussians: 0 covers every tile (more than one where the image has them), the rest are scattered; opacities up to 0.9"""
    f = 0.9 * max(W, H) + 4.0
    rng = np.random.default_rng(410 + 100 * W + H)
    n = 40
    u, v = rng.uniform(-1, W, n), rng.uniform(-1, H, n)
    sigma = rng.uniform(0.8, 1.0 + 0.15 * max(W, H), n)
    o = rng.uniform(0.1, 0.9, n)
    u[0], v[0], sigma[0], o[0] = 0.5 * W, 0.5 * H, 2.0 * max(W, H) + 8, 0.3
    z = rng.uniform(2.0, 4.0, n)
    z[0] = 1.5
    return finish(f"size{W}x{H}", place(u, v, z, W, H, f), scales_px(rng, sigma, z, f, aniso=0.2), unit_quats(rng, n), o,
                  random_shs(rng, n), W, H, f)


LISTS = [(63, 31), (63, 62), (64, 63), (65, 63), (65, 64), (129, 63), (129, 64), (129, 128)]


def list_case(n, k):
    """one 16 x 16 tile, exactly n Gaussians that all cover it, depth increasing with the id.  All but two are faint and wide
    (sigma 25..50 px, opacity 0.006..0.009: alpha stays above 1 / 255 on the whole tile, so no pixel sits on that threshold;
    (1 - 0.009)^128 = 0.31, and 0.56 after 64 of them); instance k is a slab (sigma 100 px) at opacity 0.6, which takes EVERY
    pixel's T from above 0.5 to below it: the median of every pixel is instance k (for k = 128, the first instance of the third
    batch, the faint ones are fainter still).  The last instance is a slab at opacity 0.05: max n_contrib = n."""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(505 + 1000 * k + n)
    z = 2.0 + 0.01 * np.arange(n)
    sigma = rng.uniform(25.0, 50.0, n)
    o = rng.uniform(0.006, 0.009, n)
    if k == 128:    # 128 faint ones must leave T above 0.5: sigma 60..100 px, opacity 0.0043..0.005, (1 - 0.005)^128 = 0.526
        sigma, o = rng.uniform(60.0, 100.0, n), rng.uniform(0.0043, 0.005, n)
    sigma[n - 1], o[n - 1] = 100.0, 0.05
    sigma[k], o[k] = 100.0, 0.6
    xyz = place(rng.uniform(3, 12, n), rng.uniform(3, 12, n), z, W, H, f)
    return finish(f"list{n}_{k}", xyz, scales_px(rng, sigma, z, f, aniso=0.15), unit_quats(rng, n), o, random_shs(rng, n), W, H, f)


def sat_case():
    """32 x 16, two tiles.  8 strong Gaussians (sigma 2.5..3.2 px, opacity 0.9 / 1.0) clustered in the left tile: the pixels there
    saturate early and the cap binds; 150 faint ones everywhere (they move the list position past 128); a cover at opacity 0.3;
    20 slabs at opacity 1.0 / 0.9..0.97: every remaining pixel saturates there."""
    W, H, f = 32, 16, 30.0
    rng = np.random.default_rng(606)
    k = [8, 150, 1, 20]
    n = sum(k)
    u = np.concatenate([rng.integers(3, 6, k[0]), rng.uniform(0, W - 1, k[1]), [15.5], rng.integers(0, W, k[3])]).astype(float)
    v = np.concatenate([rng.integers(6, 10, k[0]), rng.uniform(0, H - 1, k[1]), [7.5], rng.integers(0, H, k[3])]).astype(float)
    sigma = np.concatenate([rng.uniform(2.5, 3.2, k[0]), rng.uniform(1.0, 1.3, k[1]), [60.0], rng.uniform(80, 120, k[3])])
    slab_o = np.where(np.arange(k[3]) % 3 == 2, rng.uniform(0.9, 0.97, k[3]), 1.0)
    o = np.concatenate([np.where(np.arange(k[0]) % 2 == 0, 1.0, 0.9), rng.uniform(0.006, 0.009, k[1]), [0.3], slab_o])
    z = 2.0 + 0.01 * np.arange(n)
    return finish("sat", place(u, v, z, W, H, f), scales_px(rng, sigma, z, f, aniso=0.1), unit_quats(rng, n), o, random_shs(rng, n),
                  W, H, f)


def faint_case():
    """24 x 16: 30 Gaussians at opacity 0.02..0.06: alpha stays below 0.5 on every pixel, no pixel has a median"""
    W, H, f = 24, 16, 25.0
    rng = np.random.default_rng(808)
    n = 30
    z = rng.uniform(2.0, 4.0, n)
    return finish("faint", place(rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), z, W, H, f),
                  scales_px(rng, rng.uniform(2.0, 6.0, n), z, f), unit_quats(rng, n), rng.uniform(0.02, 0.06, n), random_shs(rng, n),
                  W, H, f)


def single_case():
    """40 x 16, three tiles: ONE Gaussian (sigma 2 px, opacity 0.8) in the left tile; the other two tiles are empty"""
    W, H, f = 40, 16, 40.0
    rng = np.random.default_rng(909)
    return finish("single", place([6.3], [7.6], [3.0], W, H, f), scales_px(rng, [2.0], [3.0], f, aniso=0.1), unit_quats(rng, 1), [0.8],
                  random_shs(rng, 1), W, H, f)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("size"):
        W, H = name[4:].split("x")
        return size_case(int(W), int(H))
    if name.startswith("list"):
        n, k = name[4:].split("_")
        return list_case(int(n), int(k))
    return dict(sat=sat_case, faint=faint_case, single=single_case)[name]()


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """-> (weights, g64, e32 per tensor, pg32 per Gaussian, aux of the fp64 run)"""
    c = case(name)
    a = c["arrays"]
    near05 = depth_statement.depth_maps(a, c["cam"], c["W"], c["H"], 1.0)["near05"]
    w = dict(c["weights"], wM=np.where(near05, np.float32(0), c["weights"]["wM"]))
    zeroed = float((c["near"] | near05).mean())
    assert zeroed <= 0.01, f"{name}: {zeroed:.2%} of the pixels sit on a threshold"
    args = (a, c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    (g64,), maps, aux = dgs.grads(*args, [w], torch.float64)
    (g32,), _, aux32 = dgs.grads(*args, [w], torch.float32)
    geom = c["geom"]
    np.testing.assert_array_equal(aux["radii"], geom["radii"])
    keep = ~c["near"]
    for k in ("radii", "rect", "tile_len"):
        np.testing.assert_array_equal(aux32[k], aux[k], err_msg=f"{name}: {k} of the fp32 statement")
    np.testing.assert_array_equal(aux32["n_contrib"][keep], aux["n_contrib"][keep])
    np.testing.assert_array_equal(aux32["median_pos"][keep & ~near05], aux["median_pos"][keep & ~near05])
    return w, g64, errors(g32, g64), per_gaussian(g32, g64), aux


@functools.lru_cache(maxsize=None)
def orders(name, back):
    """-> [(per-tensor errors, per-Gaussian errors)] of ORDERS more fp32 evaluations of the statement, a seeded pixel order
    each; ``back``: with the transmittance multiplied up from the back of the list (the order of the backward pass)"""
    c = case(name)
    w, g64, _, _, aux64 = oracle_of(name)
    args = (c["arrays"], c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"])
    out = []
    for seed in range(1, ORDERS + 1):
        (g32,), _, aux = dgs.grads(*args, [w], torch.float32, pixel_order_seed=seed, transmittance_from_back=back)
        np.testing.assert_array_equal(aux["radii"], aux64["radii"])
        out.append((errors(g32, g64), per_gaussian(g32, g64)))
    return out


def judge(name, g):
    """test_raster_backward_edges.judge on this file's statement: the bound is TOL_FACTOR x the row-by-row fp32 statement, per
    tensor and per Gaussian.  Where the kernels exceed it, THAT entry alone is judged by the worst of ORDERS more fp32
    evaluations of the statement in other pixel orders and, if that is not enough, with T built from the back of the list --
    the statement alone decides that the entry's sum is ill-conditioned.  The factor stays, no yardstick may exceed E32_CEILING,
    and every use is printed as a WIDER line."""
    w, g64, e32, pg32, _ = oracle_of(name)
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


# ---- the tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(13, 9), (17, 16)])
def test_small_and_partial_images(backend, W, H):
    name = f"size{W}x{H}"
    w, _, _, _, aux = oracle_of(name)
    rect = aux["rect"].astype(np.int64)
    area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    assert area[0] == aux["tile_len"].size, "Gaussian 0 covers every tile"
    if W > 16:
        assert area.max() > 1, "row value nine is summed over more than one slot"
    assert (aux["median_pos"] > 0).any()
    g, _, _ = hip_grads(backend, case(name), w)
    judge(name, g)


@pytest.mark.parametrize("n,k", LISTS)
def test_list_ends_and_median_positions(backend, n, k):
    name = f"list{n}_{k}"
    w, g64, _, _, aux = oracle_of(name)
    assert aux["tile_len"].tolist() == [[n]] and aux["n_contrib"].max() == n and not aux["saturated"].any()
    assert (aux["median_pos"] == k + 1).all(), "instance k is the median of every pixel"
    if n == 129 and k < 128:
        assert (aux["n_contrib"] > 128).all(), "the last contributor is two batches behind the median"
    assert np.abs(g64["mean3D"][k]).min() > 0
    g, _, _ = hip_grads(backend, case(name), w)
    judge(name, g)


def test_saturation_and_the_cap(backend):
    w, _, _, _, aux = oracle_of("sat")
    sat = aux["saturated"]
    assert sat.mean() > 0.9 and aux["capped"] >= 1 and aux["tile_len"].max() > 128
    assert (aux["median_pos"][sat] > 0).all(), "a saturated pixel has a median"
    last = aux["median_pos"] == aux["n_contrib"]
    assert (sat & last).any() and (sat & ~last).any(), "the median is the last contributor before the stop on some pixels only"
    assert (aux["n_contrib"][sat] < aux["tile_len"].max()).all()
    g, _, _ = hip_grads(backend, case("sat"), w)
    judge("sat", g)


def test_pixels_without_a_median_ignore_the_median_gradient(backend):
    w, g64, _, _, aux = oracle_of("faint")
    assert (aux["median_pos"] == 0).all() and (aux["n_contrib"] > 0).mean() > 0.5
    c = case("faint")
    g, _, _ = hip_grads(backend, c, w)
    judge("faint", g)
    other, _, _ = hip_grads(backend, c, dict(w, wM=np.full_like(w["wM"], 1e6)))
    for key in g:
        if g[key] is not None:
            assert g[key].tobytes() == other[key].tobytes(), f"{key}: gM reached a pixel without a median"


def test_single_contributor_and_empty_tiles(backend):
    c = case("single")
    w, g64, _, _, aux = oracle_of("single")
    assert aux["tile_len"].tolist() == [[1, 0, 0]]
    contrib, med = aux["n_contrib"] > 0, aux["median_pos"] > 0
    assert contrib.sum() > 20 and 0 < med.sum() < contrib.sum()
    g, _, _ = hip_grads(backend, c, w)
    judge("single", g)
    # depth terms alone: expected = z whatever alpha is, so the depth term's dL/dalpha vanishes and dL/dz = sum gD + sum gM
    only = {k: w[k] for k in ("wD", "wM")}
    d, _, _ = hip_grads(backend, c, only)
    dz = float(w["wD"][contrib].astype(np.float64).sum() + w["wM"][med].astype(np.float64).sum())
    vm = np.asarray(c["cam"].world_view_transform, np.float64).reshape(16)
    scale = float(np.abs(w["wD"][contrib]).sum() + np.abs(w["wM"][med]).sum())
    # D = fmaf(w, z, 0) / w differs from z by at most one rounding: |u| <= 2^-23 |gD|, against dL/dz terms of order |gD|
    np.testing.assert_allclose(d["mean3D"][0], dz * vm[[2, 6, 10]], rtol=0, atol=1e-5 * scale)
    assert np.abs(d["opacity"]).max() <= 1e-5 * scale and np.abs(d["mean2D"]).max() <= 1e-5 * scale * max(c["W"], c["H"])
    assert not d["color"].any()
