"""gs2m_mesh_sample_count / _emit (gs2mesh_amd/csrc/mesh_sample_kernels.h): the DTU evaluation's surface sampler.
A CPU test pins the numpy statement (tests/mesh_sample_statement.py) bit for bit to the points the reference's own
sample_single_tri returned (tests/golden/dtu_sample_tri.npz, written by tests/golden/make_golden_eval.py); the back-end tests
pin the kernels to the statement bit for bit: counts, offsets and points."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_sample_statement as stmt
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import _ptr

_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_statement_equals_the_reference_sampler_bit_for_bit(golden_dir):
    g = np.load(os.path.join(golden_dir, "dtu_sample_tri.npz"))
    tris, density, counts, points = g["triangles"], float(g["density"]), g["counts"], g["points"]
    assert len(tris) >= 36 and (counts == 0).sum() >= 5 and counts.max() > 500 and counts.sum() == len(points)
    got = [stmt.sample_triangle(t[0], t[1], t[2], density) for t in tris]
    np.testing.assert_array_equal([len(p) for p in got], counts)
    np.testing.assert_array_equal(bits(np.concatenate(got, 0)), bits(points))
    # and through the mesh form: a soup of the same triangles
    c, o, p, status = stmt.sample_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3), density)
    assert status == 0
    np.testing.assert_array_equal(c, counts)
    np.testing.assert_array_equal(bits(p[3 * len(tris):]), bits(points))


def run(backend, verts, tris, density, canary=4):
    """-> (counts, offsets, points, status, total); `points` carries `canary` extra rows that must stay untouched"""
    lib = backend.lib
    v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    V, T = len(v), len(t)
    dv, dt = backend.dev(v), backend.dev(t)
    counts, offsets = backend.dev(np.full(T, 0x55555555, np.uint32)), backend.dev(np.full(T, 0x55555555, np.uint32))
    state = backend.dev(np.full(T // 4096 + 4, -1, np.int64))
    total, status = C.c_int64(-1), C.c_uint32(99)
    rc = lib.gs2m_mesh_sample_count(V, _ptr(dv), T, _ptr(dt), density, _ptr(counts), _ptr(offsets), _ptr(state), (T // 4096 + 4) * 8,
                                    C.c_void_p(0), C.byref(total), C.byref(status))
    assert rc == 0, lib.gs2m_last_error()
    n = total.value if not status.value & _lib.MESH_SAMPLE_TOTAL else 0
    points = backend.dev(np.full((V + n + canary, 3), -777.0, np.float64))
    rc = lib.gs2m_mesh_sample_emit(V, _ptr(dv), T, _ptr(dt), density, _ptr(counts), _ptr(offsets), n, _ptr(points), C.c_void_p(0))
    assert rc == 0, lib.gs2m_last_error()
    backend.sync()
    p = backend.host(points)
    assert np.all(p[V + n:] == -777.0)
    return backend.host(counts).view(np.uint32), backend.host(offsets).view(np.uint32), p[:V + n], status.value, total.value


def check(backend, key, make, density):
    if key not in _REF:
        v, t = make()
        _REF[key] = (v, t) + stmt.sample_mesh(v, t, density)
    v, t, rc, ro, rp, rstatus = _REF[key]
    c, o, p, status, total = run(backend, v, t, density)
    assert status == rstatus and total == int(rc.sum(dtype=np.int64))
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(o, ro)
    np.testing.assert_array_equal(bits(p), bits(rp))
    return c, p


def edge_mesh():
    """one triangle per edge case, as a soup; the grid counts at density 0.2 are in the test below"""
    tris = [
        [[0, 0, 0], [1, 1, 1], [2, 2, 2]],                       # zero area
        [[5, 5, 5], [5, 5, 5], [5, 5, 5]],                       # a point
        [[0, 0, 0], [0.15, 0, 0], [0, 0.15, 0]],                 # N1 = N2 = 0
        [[0, 0, 0], [0.5, 0, 0], [0.01, 0.12, 0]],               # N2 = 0, N1 > 0
        [[0, 0, 0], [0.01, 0.12, 0], [0.5, 0, 0]],               # N1 = 0, N2 > 0
        [[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0]],                 # N = 1
        [[1, 2, 3], [1.45, 2, 3], [1, 2.45, 3]],                 # N = 2
        [[0, 0, 0], [20.1, 0, 0], [0, 20.1, 0]],                 # N = 100
        [[0, 0, 0], [30.0, 0, 0], [30.0, 0.05, 0]],              # needle, both long edges at v0: N = 6
        [[0, 0, 0], [30.0, 0, 0], [0, 0.003, 0]],                # needle, the short edge at v0: N1 = 150, N2 = 0
        [[-300, 200, 650], [-299.1, 200.7, 650.2], [-300.4, 200.1, 651.3]],
    ]
    v = np.array(tris, np.float64).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def test_edge_triangles_equal_the_statement(backend):
    c, p = check(backend, "edge", edge_mesh, 0.2)
    # a right isosceles triangle of N x N keeps the nodes with i + j <= N - 2: N (N - 1) / 2 of them, none at N = 1
    assert list(c[:9]) == [0, 0, 0, 0, 0, 0, 1, 4950, 15] and c[9] == 0 and c[10] > 0
    v, _ = edge_mesh()
    g = [stmt.grid_counts(v[3 * k], v[3 * k + 1], v[3 * k + 2], 0.2) for k in range(11)]
    assert (g[8][2], g[8][3]) == (6, 6) and (g[9][2], g[9][3]) == (150, 0)
    assert g[0] is None and g[1] is None
    assert (g[2][2], g[2][3]) == (0, 0) and g[3][3] == 0 < g[3][2] and g[4][2] == 0 < g[4][3]
    assert (g[5][2], g[5][3]) == (1, 1) and (g[6][2], g[6][3]) == (2, 2) and (g[7][2], g[7][3]) == (100, 100)


def test_no_triangles_gives_the_vertices(backend):
    v = np.random.default_rng(0).normal(0, 1, (5, 3))
    c, o, p, status, total = run(backend, v, np.zeros((0, 3), np.int32), 0.2)
    assert total == 0 and status == 0 and len(c) == 0
    np.testing.assert_array_equal(bits(p), bits(v))
    c, o, p, status, total = run(backend, np.zeros((0, 3)), np.zeros((0, 3), np.int32), 0.2)
    assert total == 0 and status == 0 and p.shape == (0, 3)


def shared_vertex_mesh():
    """5000 small triangles over 2600 shared vertices: the scan crosses a 4096 tile, about a third get no sample"""
    rng = np.random.default_rng(3)
    v = rng.uniform(0, 4, (2600, 3))
    t = rng.integers(0, 2600, (5000, 1)) + rng.integers(0, 12, (5000, 3))
    t = np.minimum(t, 2599).astype(np.int32)
    v = v[np.argsort(v[:, 0])] * [100, 0.25, 0.25]             # neighbours in index are neighbours in space
    return v, t


def test_many_triangles_cross_a_scan_tile(backend):
    c, p = check(backend, "shared", shared_vertex_mesh, 0.2)
    assert len(c) == 5000 and (c == 0).sum() > 500 and (c[4096:] > 0).sum() > 100 and c.sum() > 5000


def test_an_index_out_of_range_is_flagged_and_never_dereferenced(backend):
    def make():
        v, t = edge_mesh()
        t = t.copy()
        t[5, 1] = len(v)
        t[6, 0] = -1
        t[10, 2] = 2 ** 31 - 1
        return v, t
    c, p = check(backend, "bad_index", make, 0.2)
    assert _REF["bad_index"][5] == stmt.INDEX and c[5] == c[6] == c[10] == 0 and c[7] == 4950


def test_a_triangle_above_the_grid_cap_is_flagged_and_not_sampled(backend):
    def make():
        v = np.array([[0, 0, 0], [1000.0, 0, 0], [0, 1000.0, 0], [0, 0, 0], [0.25, 0, 0], [0, 0.25, 0]])
        return v, np.arange(6, dtype=np.int32).reshape(2, 3)
    c, p = check(backend, "cap", make, 1e-3)                   # N = 840 896 per side
    assert _REF["cap"][5] == stmt.CAP and c[0] == 0 and c[1] > 0
    # just under the cap: 1023 x 1023 nodes are sampled
    v = np.array([[0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    g = stmt.grid_counts(v[0], v[1], v[2], 1.0 / 1023.5)
    assert (g[2] + 1) * (g[3] + 1) <= stmt.MAX_GRID < (g[2] + 2) * (g[3] + 2)
    check(backend, "under_cap", lambda: (v, np.arange(3, dtype=np.int32).reshape(1, 3)), 1.0 / 1023.5)


ORDINARY = [[[1, 2, 3], [1.45, 2, 3], [1, 2.45, 3]],                                    # 1 sample at density 0.2
            [[-300, 200, 650], [-299.1, 200.7, 650.2], [-300.4, 200.1, 651.3]]]         # 15


def two_triangles():
    return np.array(ORDINARY, np.float64).reshape(-1, 3), np.arange(6, dtype=np.int32).reshape(2, 3)


# thr = density * sqrt(L1 L2 / A), N = floor(L / thr).  Density 0 and the two tiny ones: N = +inf or about 1e300, (N + 1)^2 is
# not <= the cap: refused and flagged.  A negative one: N < 0; NaN: N is NaN; +inf and 1e300: N = 0, whose only node is at
# c = 0.5 / 1e-7.  All of these: an empty grid, no flag, and emit writes the vertices alone.
DENSITIES = {"zero": (0.0, stmt.CAP), "least_subnormal": (5e-324, stmt.CAP), "tiny": (1e-300, stmt.CAP), "minus_zero": (-0.0, 0),
             "negative": (-0.2, 0), "nan": (float("nan"), 0), "inf": (float("inf"), 0), "minus_inf": (float("-inf"), 0),
             "huge": (1e300, 0)}


@pytest.mark.parametrize("name", sorted(DENSITIES))
def test_a_density_that_is_not_an_ordinary_positive_number(backend, name):
    density, status = DENSITIES[name]
    c, p = check(backend, ("density", name), two_triangles, density)
    assert _REF[("density", name)][5] == status and list(c) == [0, 0]
    np.testing.assert_array_equal(bits(p), bits(two_triangles()[0]))
    if name == "zero":                                           # the same mesh still samples at an ordinary density afterwards
        c, p = check(backend, ("density", "ordinary"), two_triangles, 0.2)
        assert list(c) == [1, 15]


BAD_COORDINATES = {"nan": float("nan"), "inf": float("inf"), "minus_inf": float("-inf"), "overflowing_square": 1e200,
                   "vanishing_square": 1e-200, "capped": 1e154}


@pytest.mark.parametrize("name", sorted(BAD_COORDINATES))
def test_a_vertex_coordinate_that_is_not_an_ordinary_number(backend, name):
    """four triangles, the second with one coordinate replaced, once in each of its nine places: the others keep their
    samples and their offsets.  NaN, +-inf and 1e200 (its square overflows: L = A = +inf, thr is NaN) give an empty grid;
    1e154 still has a finite square, so N is about 1e150 and the triangle is refused; 1e-200 is simply 0 to the others."""
    def make():
        v = []
        for k in range(9):
            m = np.array([ORDINARY[0], ORDINARY[1], ORDINARY[1], ORDINARY[0]], np.float64)
            m[2] += 0.5
            m[1, k // 3, k % 3] = BAD_COORDINATES[name]
            v.append(m)
        v = np.array(v).reshape(-1, 3)
        return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    c, p = check(backend, ("coordinate", name), make, 0.2)
    status = _REF[("coordinate", name)][5]
    c = c.reshape(9, 4)
    assert np.all(c[:, [0, 2, 3]] == [1, 15, 1])
    assert status == (stmt.CAP if name == "capped" else 0)
    if name == "vanishing_square":
        assert np.all(c[:, 1] > 1000)
    else:
        assert np.all(c[:, 1] == 0)


@pytest.mark.parametrize("scale,counts", [(1e-80, [1, 15]), (1e-160, [0, 0]), (1e-312, [0, 0])])
def test_meshes_at_scales_where_products_go_subnormal(backend, scale, counts):
    """1e-80: the squares of the cross product's components are subnormal (1e-320) and the grid is that of the ordinary scale;
    1e-160: the squared edges are subnormal and those underflow, A = 0; 1e-312: the coordinates themselves are subnormal"""
    def make():
        v, t = two_triangles()
        return v * scale, t
    c, p = check(backend, ("scale", scale), make, 0.2 * scale)
    assert list(c) == counts
    v = make()[0]
    assert np.all(v != 0) and (scale > 1e-300 or np.all(np.abs(v) < np.finfo(np.float64).tiny))
    np.testing.assert_array_equal(bits(p[:6]), bits(v))


@pytest.mark.parametrize("density", [0.0, -0.2, float("nan"), float("inf"), float("-inf"), -0.0])
def test_the_python_wrapper_refuses_a_density_that_is_not_positive_and_finite(backend, density):
    from gs2mesh_amd import evaluation
    with pytest.raises(ValueError, match="density"):
        evaluation.sample_mesh(two_triangles(), density, lib=backend.lib)


def test_the_python_wrapper_raises_on_every_flag(backend):
    from gs2mesh_amd import evaluation
    v, t = edge_mesh()
    pts = evaluation.sample_mesh((v, t), 0.2, lib=backend.lib)
    backend.sync()
    np.testing.assert_array_equal(bits(pts.cpu().numpy()), bits(stmt.sample_mesh(v, t, 0.2)[2]))
    bad = t.copy()
    bad[3, 0] = 33
    with pytest.raises(ValueError, match="outside"):
        evaluation.sample_mesh((v, bad), 0.2, lib=backend.lib)
    with pytest.raises(ValueError, match="grid nodes"):
        evaluation.sample_mesh((v, t), 1e-4, lib=backend.lib)
    many = np.tile(np.array([[0, 0, 0], [100.0, 0, 0], [0, 100.0, 0]]), (6000, 1))      # 6000 x 500 000 samples
    with pytest.raises(ValueError, match="2\\^31"):
        evaluation.sample_mesh((many, np.arange(18000).reshape(-1, 3)), 0.1, lib=backend.lib)


def test_arguments(backend):
    lib = backend.lib
    v, t = edge_mesh()
    dv, dt = backend.dev(v), backend.dev(t)
    T = len(t)
    counts, offsets, state = backend.dev(np.zeros(T, np.uint32)), backend.dev(np.zeros(T, np.uint32)), backend.dev(np.zeros(4, np.int64))
    total, status = C.c_int64(0), C.c_uint32(0)

    def count(nv=len(v), pv=dv, nt=T, pt=dt, c=counts, o=offsets, s=state, sb=32):
        return lib.gs2m_mesh_sample_count(nv, _ptr(pv), nt, _ptr(pt), 0.2, _ptr(c), _ptr(o), _ptr(s), sb, C.c_void_p(0), C.byref(total),
                                          C.byref(status))
    for bad, word in ((dict(nv=-1), "vertices"), (dict(nt=-1), "triangles"), (dict(pv=None), "NULL"), (dict(pt=None), "NULL"),
                      (dict(c=None), "NULL"), (dict(o=None), "NULL"), (dict(s=None), "state"), (dict(sb=23), "state")):
        assert count(**bad) != 0, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert count() == 0 and total.value == int(stmt.sample_mesh(v, t, 0.2)[0].sum())
    pts = backend.dev(np.zeros((len(v) + max(total.value, 0), 3)))
    assert lib.gs2m_mesh_sample_emit(len(v), _ptr(dv), T, _ptr(dt), 0.2, _ptr(counts), _ptr(offsets), 2 ** 31, _ptr(pts), C.c_void_p(0)) != 0
    assert "total" in lib.gs2m_last_error().decode()
    assert lib.gs2m_mesh_sample_emit(len(v), _ptr(dv), T, _ptr(dt), 0.2, _ptr(counts), _ptr(offsets), total.value, None, C.c_void_p(0)) != 0
    assert "NULL" in lib.gs2m_last_error().decode()
    backend.sync()
