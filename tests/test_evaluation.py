"""gs2mesh_amd.evaluation on both back-ends: the nearest-neighbour wrapper against scipy's KD tree, the sampler and the
metrics on a plane whose distances are known in closed form, and the torch restatements of the reference's filters against
the reference's own numpy lines."""
import numpy as np
import pytest

from gs2mesh_amd import evaluation


def host(x):
    return x.detach().cpu().numpy()


def test_nearest_neighbors_against_a_kd_tree(backend):
    """f32-representable points, origin 0.  The bound is derived, not measured: with u = 2^-24 each of dx, dy, dz carries one
    rounding, each square one more on top of two from its operand, and the two sums one each -- a relative error of the f32 d
    of at most 5u = 3e-7 against the exact distance of the same f32 points; a minimum over such values keeps the bound.
    scipy works in f64 on the same points, so rtol 1e-6 holds with room.  The index is checked by value: d(i, idx[i])
    recomputed in f32 has the returned bits."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    r = (rng.normal(0, 1, (5000, 3)) * [3, 1, 0.2]).astype(np.float32)
    q = np.concatenate([rng.normal(0, 1, (1500, 3)) * [3, 1, 0.2], rng.uniform(-20, 20, (300, 3))]).astype(np.float32)
    kd, _ = cKDTree(r.astype(np.float64)).query(q.astype(np.float64))
    for sort in (True, False):
        d2, idx = evaluation.nearest_neighbors(backend.dev(q), backend.dev(r), sort=sort, lib=backend.lib)
        backend.sync()
        d2, idx = host(d2), host(idx)
        assert d2.dtype == np.float32 and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 5000
        np.testing.assert_allclose(d2.astype(np.float64), kd ** 2, rtol=1e-6, atol=1e-30)
        dx, dy, dz = (r[idx, k] - q[:, k] for k in range(3))
        np.testing.assert_array_equal(((dx * dx + dy * dy) + dz * dz).view(np.uint32), d2.view(np.uint32))
    d2, idx = evaluation.nearest_neighbors(backend.dev(q), backend.dev(r), lib=backend.lib, want_index=False)
    assert idx is None
    d2, idx = evaluation.nearest_neighbors(backend.dev(q[:0]), backend.dev(r), lib=backend.lib)
    assert tuple(d2.shape) == (0,) and tuple(idx.shape) == (0,)
    with pytest.raises(ValueError):
        evaluation.nearest_neighbors(backend.dev(q[:, :2]), backend.dev(r), lib=backend.lib)


def test_a_sampled_plane_against_a_lattice_above_it(backend):
    """A unit square at z = 0 sampled at density delta, a lattice of pitch h at z = 0.05 over it.  Every sample has a lattice
    point within h / 2 in x and in y; every interior lattice point has a sample within the sampler's largest gap s."""
    delta, h, z = 0.03, 0.02, 0.05
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    g = np.arange(-2, 53) * h                                             # -0.04 .. 1.04
    gt = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((55, 55), z)], -1).reshape(-1, 3)
    pts = evaluation.sample_mesh((verts, tris), delta, lib=backend.lib)
    backend.sync()
    p = host(pts)
    assert p.shape[0] > 1000 and np.all(p[:, 2] == 0) and p[:, :2].min() >= 0 and p[:, :2].max() <= 1
    # the sampler's largest gap, on the CPU: the farthest any point of a fine probe grid inside the square is from a sample
    from scipy.spatial import cKDTree
    probe = np.stack(np.meshgrid(np.linspace(0, 1, 401), np.linspace(0, 1, 401), indexing="ij"), -1).reshape(-1, 2)
    s = cKDTree(p[:, :2]).query(probe)[0].max() + 0.0025 * np.sqrt(2) / 2   # + half a probe cell's diagonal
    assert delta / 2 < s < 2 * delta
    o = np.zeros(3)
    d2s = host(evaluation._distances(pts, evaluation._tensor(gt, pts.dtype), evaluation._tensor(o, pts.dtype), True, backend.lib))
    tol = 1e-6                                                              # f32 coordinates of O(1): 5 * 2^-24 relative on d2
    assert d2s.min() >= z * (1 - tol) and d2s.max() <= np.sqrt(z * z + h * h / 2) * (1 + tol)
    interior = (gt[:, 0] >= 0) & (gt[:, 0] <= 1) & (gt[:, 1] >= 0) & (gt[:, 1] <= 1)
    s2d = host(evaluation._distances(evaluation._tensor(gt[interior], pts.dtype), pts, evaluation._tensor(o, pts.dtype), True,
                                     backend.lib))
    assert s2d.min() >= z * (1 - tol) and s2d.max() <= np.sqrt(z * z + s * s) * (1 + tol)

    m = evaluation.dtu_metrics(pts, gt[interior], origin=o, lib=backend.lib)
    assert z <= m["mean_d2s"] <= np.sqrt(z * z + h * h / 2) and z <= m["mean_s2d"] <= np.sqrt(z * z + s * s)
    assert m["overall"] == (m["mean_d2s"] + m["mean_s2d"]) / 2
    np.testing.assert_allclose(m["mean_d2s"], d2s.mean(), rtol=1e-12)
    # the default origin (the midpoint of the ground truth's box) changes the f32 coordinates, not the figures beyond f32
    m2 = evaluation.dtu_metrics(pts, gt[interior], lib=backend.lib)
    np.testing.assert_allclose([m2["mean_d2s"], m2["mean_s2d"]], [m["mean_d2s"], m["mean_s2d"]], rtol=1e-5)

    upper = np.sqrt(z * z + max(s * s, h * h / 2)) * 1.001
    f = evaluation.fscore_metrics(pts, gt[interior], [0.04, upper], origin=o, lib=backend.lib)
    low, high = f["thresholds"]["0.04"], f["thresholds"][str(upper)]
    assert low == {"accuracy": 0.0, "recall": 0.0, "F1": 0.0}              # F1 is 0, not NaN
    assert high == {"accuracy": 1.0, "recall": 1.0, "F1": 1.0}
    assert f["chamfer"] == f["pred_gt"] + f["gt_pred"]
    np.testing.assert_allclose([f["pred_gt"], f["gt_pred"]], [m["mean_d2s"], m["mean_s2d"]], rtol=1e-12)

    e = evaluation.evaluate_mesh((verts, tris), gt[interior], density=delta, max_dist=20, thresholds=[0.04], origin=o, lib=backend.lib)
    assert e["n_sampled"] == p.shape[0] and 0 < e["n_thinned"] <= e["n_sampled"] and e["n_observed"] == e["n_thinned"]
    assert z <= e["mean_d2s"] <= np.sqrt(z * z + h * h / 2) and e["fscore"]["thresholds"]["0.04"]["F1"] == 0.0


def test_dtu_metrics_leaves_out_a_distance_equal_to_max_dist(backend):
    """distances 3, 4 (exactly: 3-4-5 triangles in f32) and 12; max_dist = 4 keeps the 3 alone"""
    pred = np.array([[0, 0, 3.0], [100, 0, 4.0], [200, 0, 12.0]])
    gt = np.array([[0, 0, 0.0], [100, 0, 0], [200, 0, 0]])
    o = np.zeros(3)
    m = evaluation.dtu_metrics(backend.dev(pred), backend.dev(gt), max_dist=4.0, origin=o, lib=backend.lib)
    assert m == {"mean_d2s": 3.0, "mean_s2d": 3.0, "overall": 3.0}
    m = evaluation.dtu_metrics(backend.dev(pred), backend.dev(gt), max_dist=4.0 + 1e-9, origin=o, lib=backend.lib)
    assert m["mean_d2s"] == 3.5
    m = evaluation.dtu_metrics(backend.dev(pred), backend.dev(gt), max_dist=20, origin=o, lib=backend.lib)
    assert m["mean_d2s"] == 19.0 / 3
    m = evaluation.dtu_metrics(backend.dev(pred), backend.dev(gt), max_dist=1.0, origin=o, lib=backend.lib)
    assert np.isnan(m["mean_d2s"]) and np.isnan(m["overall"])
    # the two optional sets: GT queries and prediction references of their own
    m = evaluation.dtu_metrics(backend.dev(pred[:1]), backend.dev(gt), max_dist=20, pred_refs=backend.dev(pred), gt_queries=backend.dev(gt[2:]),
                               origin=o, lib=backend.lib)
    assert m["mean_d2s"] == 3.0 and m["mean_s2d"] == 12.0


def test_thin_points_keeps_the_lowest_index_of_every_cell(backend):
    rng = np.random.default_rng(4)
    p = rng.uniform(-3, 5, (4000, 3))
    p[100:200] = p[:100] + 1e-9                                            # near-duplicates: the same cells as rows 0..99
    cell = 0.7
    got, keep = evaluation.thin_points(backend.dev(p), cell, return_index=True)
    got, keep = host(got), host(keep)
    ijk = np.floor(p / cell).astype(np.int64)
    first = {}
    for n, c in enumerate(map(tuple, ijk)):
        first.setdefault(c, n)
    want = np.array(sorted(first.values()))
    np.testing.assert_array_equal(keep, want)
    np.testing.assert_array_equal(got, p[want])
    assert len(want) < 4000 and not np.any((keep >= 100) & (keep < 200))
    assert tuple(evaluation.thin_points(backend.dev(p[:0]), cell).shape) == (0, 3)


def test_the_dtu_filters_equal_the_reference_lines_in_numpy(backend):
    rng = np.random.default_rng(5)
    ObsMask = rng.integers(0, 2, (23, 17, 29)).astype(np.uint8)
    BB = np.array([[-11.3, 4.7, 100.1], [80.9, 72.5, 215.3]])
    Res = np.array([[4.0]])
    patch = 6.0
    data_down = rng.uniform(BB[0] - 30, BB[1] + 30, (6000, 3))
    data_down[:50] = BB.astype(np.float32)[0].astype(np.float64) + rng.integers(0, 15, (50, 3)) * 4.0 + 2.0   # ties of around()
    # eval.py:100-110, the reference's own lines
    BBf = BB.astype(np.float32)
    inbound = ((data_down >= BBf[:1] - patch) & (data_down < BBf[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BBf[:1]) / Res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(ObsMask.shape, 0))).sum(axis=-1) == 3
    data_grid_in = data_grid[grid_inbound]
    in_obs = ObsMask[data_grid_in[:, 0], data_grid_in[:, 1], data_grid_in[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]

    got_in, got_obs = evaluation.dtu_observation_filter(backend.dev(data_down), ObsMask, BB, Res, patch)
    np.testing.assert_array_equal(host(got_in), inbound)
    np.testing.assert_array_equal(data_down[host(got_obs)], data_in_obs)
    assert 100 < len(data_in_obs) < inbound.sum() < 6000

    # eval.py:128-130
    stl = rng.normal(0, 50, (3000, 3))
    ground_plane = np.array([[0.02], [-0.01], [1.0], [3.5]])
    stl_hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (ground_plane.reshape((1, 4)) * stl_hom).sum(-1) > 0
    np.testing.assert_array_equal(host(evaluation.above_plane(backend.dev(stl), ground_plane)), above)
    assert 500 < above.sum() < 2500
