"""gs2m_nn_dist2 (gs2mesh_amd/csrc/nn_kernels.h) against the plain numpy statement of its arithmetic and selection rule
(tests/nn_statement.py) on both back-ends.  Every comparison is exact: the distance bit for bit and the index, whatever the
order the two sets are walked in."""
import ctypes as C

import numpy as np
import pytest

import nn_statement
from gs2mesh_amd.rasterizer import _ptr, morton_order

_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def uniform(P, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (P, 3)).astype(np.float32)


def statement(key, make):
    """(queries, refs, statement d2, statement idx), computed once per case and shared between the back-ends; never modified"""
    if key not in _REF:
        q, r = make()
        _REF[key] = (q, r) + nn_statement.nn_dist2(q, r)
    return _REF[key]


def run(backend, q, r, qo=None, ro=None, want_idx=True, fill=None):
    lib = backend.lib
    Q, R = len(q), len(r)
    need = lib.gs2m_nn_scratch_bytes(Q, R)
    scratch = backend.dev(np.zeros(need // 8 + 2, np.int64))
    d2 = backend.dev(np.full(Q, 7.0 if fill is None else fill, np.float32))
    idx = backend.dev(np.full(Q, -7, np.int32)) if want_idx else None
    dq, dr, dqo, dro = backend.dev(q), backend.dev(r), backend.dev(qo), backend.dev(ro)    # alive until the kernel has run
    rc = lib.gs2m_nn_dist2(Q, _ptr(dq), _ptr(dqo), R, _ptr(dr), _ptr(dro), _ptr(scratch), need, _ptr(d2), _ptr(idx), C.c_void_p(0))
    assert rc == 0, lib.gs2m_last_error()
    backend.sync()
    return backend.host(d2), backend.host(idx)


def morton(p):
    return morton_order(np.nan_to_num(p))                     # any permutation serves; NaN has no place on the curve


def auto(p):
    return morton(p) if len(p) >= 1024 else None


def check(backend, key, make, qo="auto", ro="auto"):
    q, r, ref_d, ref_i = statement(key, make)
    d, i = run(backend, q, r, auto(q) if isinstance(qo, str) else qo, auto(r) if isinstance(ro, str) else ro)
    assert d.dtype == np.float32 and d.shape == (len(q),) and i.dtype == np.int32 and i.shape == (len(q),)
    np.testing.assert_array_equal(bits(d), bits(ref_d))
    np.testing.assert_array_equal(i, ref_i)
    assert np.all((i >= -1) & (i < max(len(r), 1)))
    return q, r, d, i


# every R once (group of 256, super-box of 16 groups, partial last group), every Q once (wave of 64, workgroup of 4 waves)
SHAPES = [(1, 1), (63, 2), (64, 255), (65, 256), (255, 257), (256, 4095), (257, 4096), (1000, 4097), (65, 8193), (1000, 8193)]


@pytest.mark.parametrize("Q,R", SHAPES)
def test_uniform_points_equal_the_statement(backend, Q, R):
    _, _, d, i = check(backend, ("uniform", Q, R), lambda: (uniform(Q, 1000 + Q), uniform(R, R)))
    assert np.all(i >= 0) and np.all(d < 12.0)


def test_no_queries_leaves_the_outputs_untouched(backend):
    d, i = run(backend, np.zeros((0, 3), np.float32), uniform(300, 1))
    assert d.shape == (0,)
    lib = backend.lib
    d2, idx = backend.dev(np.full(5, 7.0, np.float32)), backend.dev(np.full(5, -7, np.int32))
    dr = backend.dev(uniform(300, 1))
    assert lib.gs2m_nn_dist2(0, None, None, 300, _ptr(dr), None, None, 0, _ptr(d2), _ptr(idx), C.c_void_p(0)) == 0
    backend.sync()
    assert np.all(backend.host(d2) == 7.0) and np.all(backend.host(idx) == -7)


@pytest.mark.parametrize("Q", [1, 300])
def test_no_references_give_infinity_and_no_index(backend, Q):
    d, i = run(backend, uniform(Q, 2), np.zeros((0, 3), np.float32))
    assert np.all(np.isposinf(d)) and np.all(i == -1)


def same_points():
    r = np.ascontiguousarray(np.tile(uniform(450, 2), (3, 1)))
    return r.copy(), r


def lattice_centres():
    g = np.arange(8, dtype=np.float32) * np.float32(0.25)
    r = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    c = g[:7] + np.float32(0.125)
    q = np.ascontiguousarray(np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3))
    return q, r


def clusters():
    rng = np.random.default_rng(1)

    def one(n):
        a = rng.normal(0, 0.01, (n, 3))
        b = rng.normal(0, 0.01, (n - 100, 3)) + [5, 0, 0]
        far = rng.uniform(-1, 1, (7, 3)) * 1000 + [0, 3000, 0]
        p = np.concatenate([a, b, far]).astype(np.float32)
        return p[rng.permutation(len(p))]
    return one(400), one(700)


def planar():
    q, r = uniform(700, 3), uniform(1300, 4)
    q[:, 2] = 0
    r[:, 2] = 0
    return q, r


def shifted():
    return (uniform(500, 5) + np.float32(1e4)).astype(np.float32), (uniform(900, 6) + np.float32(1e4)).astype(np.float32)


def outside():
    return (uniform(300, 7) * np.float32(0.1) + np.float32([3, -2, 5])).astype(np.float32), uniform(2000, 8)


def too_far():
    return (uniform(100, 9) + np.float32(1e30)).astype(np.float32), uniform(600, 10)


def nan_refs():
    r = uniform(1500, 11)
    rng = np.random.default_rng(12)
    bad = rng.choice(1500, 200, replace=False)
    r[bad, rng.integers(0, 3, 200)] = np.nan
    r[256:512] = np.nan                                        # a whole group
    q = np.concatenate([uniform(300, 13), r[bad[:50]], r[[0, 1, 2]]]).astype(np.float32)
    return q, r


def nan_queries():
    q = uniform(200, 14)
    q[[0, 63, 64, 130], [0, 1, 2, 0]] = np.nan
    q[131] = np.nan
    return q, uniform(700, 15)


def inf_refs():
    r = uniform(1500, 16)
    r[[0, 7, 300, 1499], [0, 1, 2, 0]] = [np.inf, -np.inf, np.inf, -np.inf]     # single coordinates
    r[256:512, 1] = np.inf                                       # a whole group: its box is at infinity in y
    return uniform(300, 17), r


def inf_queries():
    q = uniform(200, 18)
    q[0] = [np.inf, 0, 0]
    q[[63, 64, 130], [1, 2, 0]] = [-np.inf, np.inf, -np.inf]
    q[131] = np.inf
    r = uniform(700, 19)
    r[0, 0] = np.inf                                             # inf - inf: a NaN d to the queries at +inf in x
    r[300, 2] = -np.inf
    return q, r


SETS = {"same_points": same_points, "lattice_centres": lattice_centres, "clusters": clusters, "planar": planar,
        "shifted": shifted, "outside": outside, "too_far": too_far, "nan_refs": nan_refs, "nan_queries": nan_queries,
        "inf_refs": inf_refs, "inf_queries": inf_queries}


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("sort", [False, True])
def test_point_sets_that_stress_culling_ties_and_non_finite_values(backend, name, sort):
    q, r, _, _ = statement(name, SETS[name])
    q, r, d, i = check(backend, name, SETS[name], morton(q) if sort else None, morton(r) if sort else None)
    if name == "same_points":
        assert np.all(d == 0) and np.array_equal(i, np.arange(1350) % 450)       # the smallest copy's index
    if name == "lattice_centres":
        assert np.all(d == np.float32(3 * 0.125 ** 2))                              # eight exact ties
        c = (q / np.float32(0.25)).astype(np.int64)                                 # the corner with the smallest index
        assert np.array_equal(i, (c[:, 0] * 8 + c[:, 1]) * 8 + c[:, 2])
    if name == "too_far":
        assert np.all(np.isposinf(d)) and np.all(i == 0)                            # +inf with a valid index: the smallest
    if name == "nan_refs":
        ok = ~np.isnan(q).any(axis=1)                                               # 50 queries are NaN references themselves
        assert (~ok).sum() >= 50 and np.all(i[~ok] == -1)
        assert np.all(i[ok] >= 0) and not np.any(np.isnan(r[i[ok]]))                # a NaN reference is never returned
        assert np.all(np.isfinite(d[ok]))
    if name == "nan_queries":
        bad = np.isnan(q).any(axis=1)
        assert bad.sum() == 5 and np.all(np.isposinf(d[bad])) and np.all(i[bad] == -1) and np.all(i[~bad] >= 0)
    if name == "inf_refs":
        assert np.all(np.isfinite(d)) and np.all(i >= 0) and np.all(np.isfinite(r[i]))       # an infinite reference is never the nearest
    if name == "inf_queries":
        bad = np.isinf(q).any(axis=1)
        assert bad.sum() == 5 and np.all(np.isposinf(d[bad])) and np.all(np.isfinite(d[~bad]))
        # +inf with a valid index: the smallest whose d is not NaN.  Reference 0 is at +inf in x, like queries 0 and 131
        assert list(i[[0, 63, 64, 130, 131]]) == [1, 0, 0, 0, 1]


def test_the_orders_never_change_a_bit(backend):
    key, make = ("uniform", 1000, 4097), lambda: (uniform(1000, 2000), uniform(4097, 4097))
    q, r, _, _ = statement(key, make)

    def orders(p, seed):
        m = morton(p)
        return {"none": None, "morton": m, "reversed": np.ascontiguousarray(m[::-1]),
                "random": np.random.default_rng(seed).permutation(len(p)).astype(np.int32)}
    for nq, qo in orders(q, 9).items():
        for nr, ro in orders(r, 10).items():
            check(backend, key, make, qo, ro)
    q, r, _, _ = statement("lattice_centres", lattice_centres)
    for nr, ro in orders(r, 11).items():
        check(backend, "lattice_centres", lattice_centres, None, ro)


def test_out_of_range_order_entries_stay_inside_the_arrays(backend):
    """a broken precondition gives unspecified values, never an access outside the arrays"""
    q, r = uniform(300, 5), uniform(600, 6)
    qo, ro = np.arange(300, dtype=np.int32), np.arange(600, dtype=np.int32)
    qo[[0, 17, 299]] = [-1, 300, 2 ** 31 - 1]
    ro[[0, 17, 599]] = [-1, 600, 2 ** 31 - 1]
    d, i = run(backend, q, r, qo, ro)
    assert np.all(np.isfinite(d)) and np.all((i >= 0) & (i < 600))


def test_the_index_output_is_optional(backend):
    q, r, ref_d, _ = statement(("uniform", 257, 4096), lambda: (uniform(257, 1257), uniform(4096, 4096)))
    d, i = run(backend, q, r, want_idx=False)
    assert i is None
    np.testing.assert_array_equal(bits(d), bits(ref_d))


def test_arguments_and_no_state_between_calls(backend):
    lib = backend.lib
    Q, R = 255, 257
    q, r, ref_d, ref_i = statement(("uniform", Q, R), lambda: (uniform(Q, 1000 + Q), uniform(R, R)))
    need = lib.gs2m_nn_scratch_bytes(Q, R)
    assert need >= 16 * R and lib.gs2m_nn_scratch_bytes(Q, 0) == 0 and lib.gs2m_nn_scratch_bytes(0, R) == need
    assert lib.gs2m_nn_scratch_bytes(1, 2 ** 31 - 1) > 16 * (2 ** 31 - 1)                # 64-bit size
    scratch = backend.dev(np.zeros(need // 8 + 1, np.int64))
    dq, dr = backend.dev(q), backend.dev(r)
    d2, idx = backend.dev(np.full(Q, 7.0, np.float32)), backend.dev(np.full(Q, -7, np.int32))
    st = C.c_void_p(0)

    def call(nq=Q, pq=dq, nr=R, pr=dr, sc=scratch, nbytes=need, od=d2, oi=idx):
        return lib.gs2m_nn_dist2(nq, _ptr(pq), None, nr, _ptr(pr), None, _ptr(sc), nbytes, _ptr(od), _ptr(oi), st)

    for bad, word in ((dict(nbytes=need - 1), "scratch"), (dict(sc=None), "scratch"), (dict(pq=None), "NULL"), (dict(pr=None), "NULL"),
                      (dict(od=None), "NULL"), (dict(nq=-1), "Q = -1"), (dict(nr=-1), "R = -1")):
        assert call(**bad) != 0, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert call(nq=0) == 0 and call(nq=0, pq=None, pr=None, sc=None, nbytes=0, od=None, oi=None) == 0
    backend.sync()
    assert np.all(backend.host(d2) == 7.0) and np.all(backend.host(idx) == -7)          # Q = 0: outputs untouched
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(d2)), bits(ref_d))
    np.testing.assert_array_equal(backend.host(idx), ref_i)
    # the same scratch, other sizes: that call's own result
    q2, r2, ref_d2, ref_i2 = statement(("uniform", 64, 255), lambda: (uniform(64, 1064), uniform(255, 255)))
    d22, idx2 = backend.dev(np.zeros(64, np.float32)), backend.dev(np.zeros(64, np.int32))
    dq2, dr2 = backend.dev(q2), backend.dev(r2)
    assert call(nq=64, pq=dq2, nr=255, pr=dr2, od=d22, oi=idx2) == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(d22)), bits(ref_d2))
    np.testing.assert_array_equal(backend.host(idx2), ref_i2)
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(d2)), bits(ref_d))
    np.testing.assert_array_equal(backend.host(idx), ref_i)
