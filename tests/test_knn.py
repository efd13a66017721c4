"""gs2m_knn_mean_dist2 (gs2mesh_amd/csrc/knn_kernels.h) against the plain numpy statement of its arithmetic
(tests/knn_statement.py) on both back-ends.  Every comparison is bit for bit: the kernel computes the exact 3-NN in the
statement's f32 arithmetic, whatever the order it walks the points in."""
import ctypes as C

import numpy as np
import pytest

import knn_statement
from gs2mesh_amd.rasterizer import _ptr, morton_order
from gs2mesh_amd.simple_knn._C import knn_mean_dist2

_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def uniform(P, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (P, 3)).astype(np.float32)


def statement(key, make):
    """(points, statement result), computed once per point set and shared between the back-ends; never modified"""
    if key not in _REF:
        pts = make()
        ref = knn_statement.mean_dist2(pts)
        _REF[key] = (pts, ref)
    return _REF[key]


def run(backend, pts, order=None):
    out = knn_mean_dist2(backend.dev(pts), None if order is None else backend.dev(order), lib=backend.lib)
    backend.sync()
    return backend.host(out)


def auto_order(pts):
    return morton_order(pts) if pts.shape[0] >= 1024 else None


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 255, 256, 257, 1000, 4097, 8193])
def test_uniform_points_equal_the_statement(backend, P):
    pts, ref = statement(("uniform", P), lambda: uniform(P, P))
    got = run(backend, pts, auto_order(pts))
    assert got.dtype == np.float32 and got.shape == (P,)
    np.testing.assert_array_equal(bits(got), bits(ref))
    if P <= 2:
        assert np.all(np.isposinf(got))
    if P == 3:
        assert np.all(got > 1.1e38) and np.all(np.isfinite(got))        # (d0 + d1 + FLT_MAX) / 3
    if P >= 4:
        assert np.all(got < 12.0)


def clusters():
    r = np.random.default_rng(1)
    a = r.normal(0, 0.01, (600, 3))
    b = r.normal(0, 0.01, (500, 3)) + [5, 0, 0]
    far = r.uniform(-1, 1, (7, 3)) * 1000 + [0, 3000, 0]
    p = np.concatenate([a, b, far]).astype(np.float32)
    return p[r.permutation(len(p))]


def repeated():
    return np.ascontiguousarray(np.tile(uniform(150, 2), (4, 1)))


def lattice():
    g = np.arange(8, dtype=np.float32) * np.float32(0.25)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def planar():
    p = uniform(1300, 3)
    p[:, 2] = 0
    return p


def shifted():
    return (uniform(900, 4) + np.float32(1e4)).astype(np.float32)


SETS = {"clusters": clusters, "repeated": repeated, "lattice": lattice, "planar": planar, "shifted": shifted}


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("sort", [False, True])
def test_point_sets_that_stress_culling_and_ties(backend, name, sort):
    pts, ref = statement(name, SETS[name])
    got = run(backend, pts, morton_order(pts) if sort else None)
    np.testing.assert_array_equal(bits(got), bits(ref))
    if name == "repeated":
        assert len(got) == 600 and np.all(got == 0)                     # three exact copies of every point
    if name == "lattice":
        assert np.all(got == np.float32(0.0625))                        # three neighbours at one step in every corner too


def test_the_order_never_changes_a_bit(backend):
    pts, ref = statement(("uniform", 4097), lambda: uniform(4097, 4097))
    m = morton_order(pts)
    orders = {"none": None, "morton": m, "reversed": np.ascontiguousarray(m[::-1]),
              "random": np.random.default_rng(9).permutation(4097).astype(np.int32)}
    for name, o in orders.items():
        np.testing.assert_array_equal(bits(run(backend, pts, o)), bits(ref), err_msg=name)


def test_out_of_range_order_entries_stay_inside_the_arrays(backend):
    """a broken precondition gives unspecified values, never an access outside [0, P)"""
    pts = uniform(300, 5)
    order = np.arange(300, dtype=np.int32)
    order[[0, 17, 299]] = [-1, 300, 2 ** 31 - 1]
    got = run(backend, pts, order)
    assert got.shape == (300,) and np.all(np.isfinite(got))


def test_arguments_and_no_state_between_calls(backend):
    lib = backend.lib
    P = 700
    pts, ref = statement(("uniform", P), lambda: uniform(P, P))
    need = lib.gs2m_knn_scratch_bytes(P)
    assert need >= 16 * P and lib.gs2m_knn_scratch_bytes(0) == 0
    assert lib.gs2m_knn_scratch_bytes(2 ** 31 - 1) > 16 * (2 ** 31 - 1)                 # 64-bit size
    scratch = backend.dev(np.zeros(need // 8 + 1, np.int64))
    dp = backend.dev(pts)
    out = backend.dev(np.full(P, 7.0, np.float32))
    st = C.c_void_p(0)

    def call(n=P, p=dp, sc=scratch, nbytes=need, o=out):
        return lib.gs2m_knn_mean_dist2(n, _ptr(p), None, _ptr(sc), nbytes, _ptr(o), st)

    for bad, word in ((dict(nbytes=need - 1), "scratch"), (dict(sc=None), "scratch"), (dict(p=None), "NULL"),
                      (dict(o=None), "NULL"), (dict(n=-1), "P = -1")):
        assert call(**bad) != 0, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert call(n=0) == 0 and call(n=0, p=None, sc=None, nbytes=0, o=None) == 0
    backend.sync()
    assert np.all(backend.host(out) == 7.0)                                             # P = 0: out untouched
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(out)), bits(ref))
    # the same scratch, another P: that call's own result
    P2 = 257
    pts2, ref2 = statement(("uniform", P2), lambda: uniform(P2, P2))
    out2 = backend.dev(np.zeros(P2, np.float32))
    assert call(n=P2, p=backend.dev(pts2), o=out2) == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(out2)), bits(ref2))
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(out)), bits(ref))
