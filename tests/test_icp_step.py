"""gs2m_icp_prepare / gs2m_icp_step (gs2mesh_amd/csrc/icp_kernels.h) against the plain numpy statement of their arithmetic, search
rule and reduction tree (tests/icp_statement.py) on both back-ends.  Every comparison is exact: the pair count, the seventeen
f64 sums bit for bit, every index and every f64 squared distance, whatever order the two sets are walked in."""
import ctypes as C

import numpy as np
import pytest

import icp_statement
from gs2mesh_amd.rasterizer import _ptr, morton_order

_REF = {}
ORIGIN = np.array([0.1, -0.2, 0.05])


def rigid(angle=0.3, axis=(1.0, 2.0, -1.0), t=(0.05, -0.02, 0.03), scale=1.0):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K))
    T[:3, 3] = t
    return T


def uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3))


def host_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def morton(p):
    return morton_order(np.nan_to_num(np.asarray(p, np.float64)).astype(np.float32))


def run(backend, source, T, target, origin, max_dist, qo=None, ro=None, want=True, calls=1):
    """-> (n, sums [17] f64, idx, d2) of the last of `calls` steps after one prepare"""
    lib = backend.lib
    source, target = np.ascontiguousarray(source, np.float64).reshape(-1, 3), np.ascontiguousarray(target, np.float64).reshape(-1, 3)
    N, R = len(source), len(target)
    need = lib.gs2m_icp_scratch_bytes(N, R)
    scratch = backend.dev(np.zeros(need // 8 + 2, np.int64))
    ds, dt, dqo, dro = backend.dev(source), backend.dev(target), backend.dev(qo), backend.dev(ro)
    Th, oh = np.ascontiguousarray(T, np.float64), np.ascontiguousarray(origin, np.float64)
    st = C.c_void_p(0)
    assert lib.gs2m_icp_prepare(R, _ptr(dt), host_ptr(oh), _ptr(dro), _ptr(scratch), need, st) == 0, lib.gs2m_last_error()
    for _ in range(calls):
        sums = backend.dev(np.full(18, 7, np.int64))
        idx = backend.dev(np.full(N, -7, np.int32)) if want else None
        d2 = backend.dev(np.full(N, 7.0, np.float64)) if want else None
        rc = lib.gs2m_icp_step(N, _ptr(ds), _ptr(dqo), host_ptr(Th), R, _ptr(dt), host_ptr(oh), float(max_dist), _ptr(scratch), need,
                               _ptr(sums), _ptr(idx), _ptr(d2), st)
        assert rc == 0, lib.gs2m_last_error()
    backend.sync()
    raw = backend.host(sums)
    return int(raw[0]), raw[1:].copy().view(np.float64), backend.host(idx), backend.host(d2)


def statement(key, make):
    """the case's inputs and its statement, computed once, shared between the back-ends and never modified"""
    if key not in _REF:
        args = make()
        _REF[key] = (args, icp_statement.icp_step(*args))
    return _REF[key]


def same(got, ref):
    n, sums, idx, d2 = got
    assert n == ref["n"]
    np.testing.assert_array_equal(sums.view(np.uint64), ref["sums"].view(np.uint64))
    if idx is not None:
        np.testing.assert_array_equal(idx, ref["idx"])
        np.testing.assert_array_equal(d2.view(np.uint64), ref["d2"].view(np.uint64))


def check(backend, key, make, orders=(False, True)):
    (source, T, target, origin, max_dist), ref = statement(key, make)
    for sort in orders:
        qo = morton(source) if sort and len(source) else None
        ro = morton(target) if sort and len(target) else None
        same(run(backend, source, T, target, origin, max_dist, qo, ro), ref)
    return ref


# every N once (wave of 64, workgroup of 256, chunk of 1024, more than 256 chunks = a thread of the last stage adds two partials),
# every R once (group of 256, super-box of 16 groups)
SHAPES = [(1, 1, 2.0), (63, 255, 0.25), (64, 256, 0.25), (65, 4097, 0.08), (255, 1, 1.2), (256, 255, 0.25), (257, 256, 0.25),
          (1025, 4097, 0.08), (2500, 256, 0.25), (256 * 1024 + 1030, 1, 1.2)]


@pytest.mark.parametrize("N,R,max_dist", SHAPES)
def test_sums_indices_and_distances_equal_the_statement_with_and_without_orders(backend, N, R, max_dist):
    ref = check(backend, ("shape", N, R), lambda: (uniform(N, N), rigid(), uniform(R, 10000 + R), ORIGIN, max_dist))
    if N > 1:
        assert 0 < ref["n"] < N                                      # the threshold cuts through the set


def test_a_pair_exactly_at_max_dist_is_left_out(backend):
    source = np.array([[0, 0, 0], [10, 0, 0.0]])
    target = np.array([[3, 4, 0], [10, 0, 2.0]])                      # d2 = 25 and 4, exact in f32 and f64
    make = lambda m: (lambda: (source, np.eye(4), target, np.zeros(3), m))
    ref = check(backend, "edge", make(5.0))
    assert ref["n"] == 1 and list(ref["d2"]) == [25.0, 4.0] and list(ref["idx"]) == [0, 1]
    assert ref["sums"][0] == 4.0
    ref = check(backend, "edge+", make(np.nextafter(5.0, 6.0)))
    assert ref["n"] == 2 and ref["sums"][0] == 29.0


def test_no_pair_and_every_pair(backend):
    make = lambda m: (lambda: (uniform(700, 1), rigid(), uniform(900, 2), ORIGIN, m))
    ref = check(backend, "none", make(1e-9))
    assert ref["n"] == 0 and not ref["sums"].any() and np.all(ref["idx"] >= 0)
    ref = check(backend, "all", make(100.0))
    assert ref["n"] == 700


def test_no_target_and_no_source(backend):
    n, sums, idx, d2 = run(backend, uniform(300, 3), rigid(), np.zeros((0, 3)), ORIGIN, 1.0)
    assert n == 0 and not sums.view(np.uint64).any() and np.all(idx == -1) and np.all(np.isposinf(d2))
    n, sums, idx, d2 = run(backend, np.zeros((0, 3)), rigid(), uniform(300, 4), ORIGIN, 1.0)
    assert n == 0 and not sums.view(np.uint64).any()                 # the 7s are gone: zero sums were written


def test_a_nan_source_row_pairs_with_nothing(backend):
    def make():
        s = uniform(300, 5)
        s[[0, 63, 64, 200], [0, 1, 2, 0]] = np.nan
        s[201] = np.nan
        return s, rigid(), uniform(500, 6), ORIGIN, 100.0
    ref = check(backend, "nan", make)
    assert ref["n"] == 295 and np.all(ref["idx"][[0, 63, 64, 200, 201]] == -1) and np.all(np.isfinite(ref["sums"]))


def test_coincident_targets_tie_to_the_smallest_index(backend):
    def make():
        t = uniform(600, 7)
        t[[17, 300, 599]] = t[5]                                     # four copies of one point
        s = np.concatenate([t[[599]], uniform(100, 8)])
        return s, np.eye(4), t, ORIGIN, 0.5
    ref = check(backend, "tie", make)
    assert ref["idx"][0] == 5 and ref["d2"][0] == 0.0


def test_two_calls_give_the_same_bits_and_the_outputs_are_optional(backend):
    (args, ref) = statement(("shape", 2500, 256), lambda: (uniform(2500, 2500), rigid(), uniform(256, 10256), ORIGIN, 0.25))
    a = run(backend, *args, calls=1)
    b = run(backend, *args, calls=3)
    same(a, ref)
    same(b, ref)
    n, sums, idx, d2 = run(backend, *args, want=False)
    assert idx is None and d2 is None
    same((n, sums, None, None), ref)


def test_arguments_are_checked(backend):
    lib = backend.lib
    N, R = 100, 300
    s, t = backend.dev(uniform(N, 1)), backend.dev(uniform(R, 2))
    need = lib.gs2m_icp_scratch_bytes(N, R)
    assert need >= 16 * R + 12 * R + 4 * N + 18 * 8 and lib.gs2m_icp_scratch_bytes(0, 0) == 0
    assert lib.gs2m_icp_scratch_bytes(0, R) < need and lib.gs2m_icp_scratch_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 32 * (2 ** 31 - 1)
    scratch, sums = backend.dev(np.zeros(need // 8 + 2, np.int64)), backend.dev(np.full(18, 7, np.int64))
    T, o = np.eye(4), np.zeros(3)
    st = C.c_void_p(0)
    assert lib.gs2m_icp_prepare(R, _ptr(t), host_ptr(o), None, _ptr(scratch), need, st) == 0

    def step(n=N, ps=s, r=R, pt=t, m=1.0, sc=scratch, nbytes=need, out=sums, pT=host_ptr(T)):
        return lib.gs2m_icp_step(n, _ptr(ps), None, pT, r, _ptr(pt), host_ptr(o), m, _ptr(sc), nbytes, _ptr(out), None, None, st)

    for m in (0.0, -1.0, float("inf"), float("nan")):
        assert step(m=m) != 0
        assert "max_dist" in lib.gs2m_last_error().decode()
    for bad, word in ((dict(nbytes=need - 1), "scratch"), (dict(sc=None), "scratch"), (dict(ps=None), "NULL"), (dict(pt=None), "NULL"),
                      (dict(out=None), "NULL"), (dict(pT=None), "NULL"), (dict(n=-1), "N = -1"), (dict(r=-1), "R = -1")):
        assert step(**bad) != 0, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert lib.gs2m_icp_prepare(R, _ptr(t), host_ptr(o), None, _ptr(scratch), lib.gs2m_icp_scratch_bytes(0, R) - 1, st) != 0
    assert "scratch" in lib.gs2m_last_error().decode()
    assert lib.gs2m_icp_prepare(-1, _ptr(t), host_ptr(o), None, _ptr(scratch), need, st) != 0
    backend.sync()
    assert np.all(backend.host(sums) == 7)                           # a refused call writes nothing
    assert step(m=100.0) == 0
    backend.sync()
    assert backend.host(sums)[0] == N
