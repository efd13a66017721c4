"""``voxel_down_sample`` / ``gs2m_voxel_mean`` bit for bit against a numpy dict loop, ``crop_points`` against an even-odd test written
another way, and TNT's whole flow (``tnt_evaluate``) on a small synthetic scene, on both back-ends."""
import ctypes as C
import json

import numpy as np
import pytest

import icp_statement
from gs2mesh_amd import evaluation
from gs2mesh_amd.rasterizer import _ptr

_REF = {}


def host(x):
    return x.detach().cpu().numpy()


# ---- voxel_down_sample -----------------------------------------------------------------------------------------------------

VOXEL = 0.5


def voxel_cloud():
    """min = (-2, -2, -2), so the voxel faces lie at -2.25 + 0.5 k, exact in binary.  Cells far from the rest hold exactly 1, 2,
    64, 65 and 1000 points; 600 more points straddle the origin (negative coordinates), 200 lie on voxel faces."""
    rng = np.random.default_rng(0)
    parts = [np.array([[-2.0, -2.0, -2.0]])]
    for cell, count in (((10, 3, 4), 1), ((11, 7, 2), 2), ((3, 12, 9), 64), ((14, 14, 1), 65), ((8, 1, 13), 1000)):
        parts.append(-2.25 + VOXEL * (np.array(cell) + rng.uniform(0.05, 0.95, (count, 3))))
    parts.append(rng.uniform(-1.9, 1.0, (600, 3)))
    faces = rng.uniform(-1.9, 1.0, (200, 3))
    on = rng.integers(0, 3, 200)
    faces[np.arange(200), on] = -2.25 + VOXEL * rng.integers(1, 6, 200)
    parts.append(faces)
    p = np.concatenate(parts)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def dict_loop(p, voxel):
    """Open3D's VoxelDownSample in plain Python: key = floor((p - (min - voxel / 2)) / voxel), the points of a voxel added in
    index order, divided by their number; here listed in ascending key"""
    lo = p.min(0) - voxel * 0.5
    acc, cnt = {}, {}
    for row in p:
        k = tuple(np.floor((row - lo) / voxel).astype(np.int64))
        if k not in acc:
            acc[k], cnt[k] = np.zeros(3), 0
        acc[k] = acc[k] + row
        cnt[k] += 1
    keys = sorted(acc)
    return np.stack([acc[k] / np.float64(cnt[k]) for k in keys]), [cnt[k] for k in keys]


def test_voxel_down_sample_equals_the_dict_loop_bit_for_bit(backend):
    if "voxel" not in _REF:
        p = voxel_cloud()
        _REF["voxel"] = (p,) + dict_loop(p, VOXEL)
    p, want, counts = _REF["voxel"]
    assert {1, 2, 64, 65, 1000} <= set(counts) and p.min() == -2.0
    got = evaluation.voxel_down_sample(backend.dev(p), VOXEL, lib=backend.lib)
    backend.sync()
    got = host(got)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    assert tuple(evaluation.voxel_down_sample(backend.dev(p[:0]), VOXEL, lib=backend.lib).shape) == (0, 3)
    one = host(evaluation.voxel_down_sample(backend.dev(p[:1]), VOXEL, lib=backend.lib))
    assert np.array_equal(one, p[:1])
    with pytest.raises(ValueError):
        evaluation.voxel_down_sample(backend.dev(p), 0.0, lib=backend.lib)


def test_voxel_mean_adds_in_the_order_given(backend):
    """the kernel alone, against tests/icp_statement.py: any order, segments of 1, 2, 64, 65 and 1000 rows, and a last one that
    runs to the end"""
    rng = np.random.default_rng(1)
    n = 1 + 2 + 64 + 65 + 1000 + 37
    p = rng.normal(0, 100, (n, 3)) * [1, 1e-3, 1e3]
    order = rng.permutation(n).astype(np.int32)
    heads = np.cumsum([0, 1, 2, 64, 65, 1000]).astype(np.int32)
    want = icp_statement.voxel_mean(p, order, heads)
    lib = backend.lib
    dp, do, dh = backend.dev(p), backend.dev(order), backend.dev(heads)
    means = backend.dev(np.full((len(heads), 3), 7.0))
    assert lib.gs2m_voxel_mean(n, _ptr(dp), _ptr(do), len(heads), _ptr(dh), _ptr(means), C.c_void_p(0)) == 0, lib.gs2m_last_error()
    backend.sync()
    np.testing.assert_array_equal(backend.host(means).view(np.uint64), want.view(np.uint64))
    assert lib.gs2m_voxel_mean(n, _ptr(dp), _ptr(do), 0, None, None, C.c_void_p(0)) == 0             # no segments: nothing to do
    assert lib.gs2m_voxel_mean(-1, _ptr(dp), _ptr(do), 1, _ptr(dh), _ptr(means), C.c_void_p(0)) != 0
    assert lib.gs2m_voxel_mean(n, None, _ptr(do), 1, _ptr(dh), _ptr(means), C.c_void_p(0)) != 0
    assert "NULL" in lib.gs2m_last_error().decode()


def test_uniform_down_sample_takes_every_kth_row(backend):
    p = np.arange(30, dtype=np.float64).reshape(10, 3)
    assert np.array_equal(host(evaluation.uniform_down_sample(backend.dev(p), 3)), p[::3])
    assert np.array_equal(host(evaluation.uniform_down_sample(backend.dev(p), 1)), p)


# ---- crop_points -----------------------------------------------------------------------------------------------------------

# a concave polygon (an arrow head with a notch), counter-clockwise, in the plane of the two axes that are not orthogonal
POLYGON_2D = np.array([[0.0, 0.0], [4.0, 0.5], [3.0, 2.0], [5.0, 4.0], [2.5, 3.0], [1.0, 5.0], [1.5, 2.5], [-1.0, 2.0]])


def inside_even_odd(poly, x, y):
    """the crossing-number test with the ray towards +x (crop_points counts the crossings on the other side)"""
    n = 0
    for i in range(len(poly)):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % len(poly)]
        if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
            n += 1
    return n % 2 == 1


def edge_distance(poly, x, y):
    d = np.inf
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        t = np.clip(((x - a[0]) * (b[0] - a[0]) + (y - a[1]) * (b[1] - a[1])) / ((b - a) @ (b - a)), 0, 1)
        d = min(d, np.hypot(x - (a[0] + t * (b[0] - a[0])), y - (a[1] + t * (b[1] - a[1]))))
    return d


@pytest.mark.parametrize("axis", ["x", "Y", "z"])
def test_crop_points_against_an_even_odd_test(backend, axis, tmp_path):
    w = "xyz".index(axis.lower())
    u, v = [a for a in range(3) if a != w]
    poly = np.zeros((len(POLYGON_2D), 3))
    poly[:, u], poly[:, v] = POLYGON_2D[:, 0], POLYGON_2D[:, 1]
    poly[:, w] = 123.0                                               # Open3D's files carry a value here; it is not read
    path = tmp_path / "crop.json"
    path.write_text(json.dumps({"axis_max": 1.5, "axis_min": -0.5, "bounding_polygon": poly.tolist(), "class_name": "SelectionPolygonVolume",
                                "orthogonal_axis": axis, "version_major": 1, "version_minor": 0}))
    vol = evaluation.read_crop_volume(path)
    assert vol["orthogonal_axis"] == axis.lower() and vol["axis_min"] == -0.5 and vol["bounding_polygon"].shape == (8, 3)
    rng = np.random.default_rng(2)
    q = np.zeros((3000, 3))
    q[:, u], q[:, v], q[:, w] = rng.uniform(-1.5, 5.5, 3000), rng.uniform(-0.5, 5.5, 3000), rng.uniform(-1.0, 2.0, 3000)
    q = q[[edge_distance(POLYGON_2D, x, y) > 1e-6 for x, y in zip(q[:, u], q[:, v])]]        # away from the edges
    want = np.array([inside_even_odd(POLYGON_2D, x, y) for x, y in zip(q[:, u], q[:, v])]) & (q[:, w] >= -0.5) & (q[:, w] <= 1.5)
    assert 300 < want.sum() < len(q) - 300
    mask = host(evaluation.crop_points(backend.dev(q), vol, return_mask=True))
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(host(evaluation.crop_points(backend.dev(q), vol)), q[want])
    # the notch: a point in the polygon's hull but outside it
    probe = np.zeros((2, 3))
    probe[:, u], probe[:, v] = [2.0, 4.0], [1.0, 2.5]
    assert list(host(evaluation.crop_points(backend.dev(probe), vol, return_mask=True))) == [True, False]


def test_crop_points_keeps_both_axis_bounds(backend):
    """axis_min <= p_w <= axis_max: both ends are inside, the next number beyond either is outside"""
    vol = {"orthogonal_axis": "z", "axis_min": -0.5, "axis_max": 1.5,
           "bounding_polygon": np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.0]])}
    z = np.array([-0.5, 1.5, np.nextafter(-0.5, -1), np.nextafter(1.5, 2), 0.0])
    q = np.stack([np.full(5, 0.5), np.full(5, 0.5), z], 1)
    assert list(host(evaluation.crop_points(backend.dev(q), vol, return_mask=True))) == [True, True, False, False, True]


# ---- TNT's flow ------------------------------------------------------------------------------------------------------------

def test_tnt_evaluate_recovers_the_perturbation_of_a_small_scene(backend):
    """141 x 141 = 19 881 ground-truth points of pitch h = 1 / 70 on a surface without symmetry, a crop square whose sides run
    half-way between grid lines (so the last stage sees the same points on both sides), the prediction = the ground truth
    moved by the inverse of a small similarity S.  The third stage then pairs every point with its own copy, the fit is exact
    up to rounding, and every distance of the final score is rounding too."""
    h = 1.0 / 70
    g = np.arange(-70, 71) * h
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    gt = np.stack([x, y, 0.3 * np.sin(2 * x + 0.5) * np.cos(3 * y) + 0.1 * x * y], 1)
    a = np.array([0.3, -1.0, 2.0]) / np.linalg.norm([0.3, -1.0, 2.0])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    S = np.eye(4)
    S[:3, :3] = 1.002 * (np.eye(3) + np.sin(0.004) * K + (1 - np.cos(0.004)) * (K @ K))
    S[:3, 3] = [0.003, -0.002, 0.001]
    Si = np.linalg.inv(S)
    pred = gt @ Si[:3, :3].T + Si[:3, 3]
    c = 63.5 * h
    vol = {"orthogonal_axis": "z", "axis_min": -1.0, "axis_max": 1.0,
           "bounding_polygon": np.array([[-c, -c, 0], [c, -c, 0], [c, c, 0], [-c, c, 0.0]])}
    tau = 0.02
    out = evaluation.tnt_evaluate(backend.dev(pred), backend.dev(gt), np.eye(4), vol, tau, lib=backend.lib)
    print(f"max|T - S| = {np.abs(out['transformation'] - S).max():.3e}, n = {out['n_source']}, {out['n_target']}")
    assert out["n_source"] == out["n_target"] == 127 * 127           # tau / 2 < h: a voxel holds one point
    assert np.abs(out["transformation"] - S).max() < 1e-9
    assert out["precision"] == 1.0 and out["recall"] == 1.0 and out["fscore"] == 1.0
