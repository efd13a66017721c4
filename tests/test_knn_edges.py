"""gs2m_knn_mean_dist2 (gs2mesh_amd/csrc/knn_kernels.h) on input that is not finite or not normal, and at the shapes
tests/test_knn.py leaves out, on both back-ends, bit for bit against tests/knn_statement.py.

The contract (include/gs2mesh_amd.h): a d that is NaN or not below FLT_MAX never counts.  So a point with a NaN or
infinite coordinate gets +inf and changes no other point's result, and a neighbour so far away that d overflows stands as
FLT_MAX, like a missing one.  "Changes no other point" is checked against the statement of the cloud WITHOUT the point, and
under every order: v_med3_f32 answers a NaN operand with the minimum of the other two, so a NaN candidate that reached the
triple would turn (b0, b1, b2) into (b0, b0, b1), by an amount that depends on when it is met."""
import ctypes as C

import numpy as np
import pytest

import knn_statement
from gs2mesh_amd.rasterizer import _ptr, morton_order
from gs2mesh_amd.simple_knn._C import knn_mean_dist2

FLT_MAX = knn_statement.FLT_MAX
TWO_NEIGHBOURS = FLT_MAX / np.float32(3)        # ((d0 + d1) + FLT_MAX) / 3 with d0 + d1 below half an ulp of FLT_MAX (2e31)
_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def uniform(P, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (P, 3)).astype(np.float32)


def statement(key, make):
    """(points, statement result), computed once per point set and shared between the back-ends; never modified"""
    if key not in _REF:
        pts = make()
        _REF[key] = (pts, knn_statement.mean_dist2(pts))
    return _REF[key]


def without(key, make, rows):
    """the statement of the cloud with `rows` removed, scattered back to the full numbering (+inf in the removed rows)"""
    if (key, "without") not in _REF:
        pts, _ = statement(key, make)
        keep = np.setdiff1d(np.arange(len(pts)), rows)
        full = np.full(len(pts), np.inf, np.float32)
        full[keep] = knn_statement.mean_dist2(pts[keep])
        _REF[(key, "without")] = full
    return _REF[(key, "without")]


def run(backend, pts, order=None):
    out = knn_mean_dist2(backend.dev(pts), None if order is None else backend.dev(order), lib=backend.lib)
    backend.sync()
    return backend.host(out)


def morton(p):
    return morton_order(np.nan_to_num(p, posinf=2.0, neginf=-2.0))          # any permutation serves; NaN has no place on the curve


def orders(pts, seed=9):
    m = morton(pts)
    return {"none": None, "reversed": np.ascontiguousarray(np.arange(len(pts), dtype=np.int32)[::-1]),
            "random": np.random.default_rng(seed).permutation(len(pts)).astype(np.int32), "morton": m}


def check_bad_rows(backend, key, make, rows):
    """every order gives the statement's bits; `rows` get +inf; the others what they get without `rows` in the cloud"""
    pts, ref = statement(key, make)
    alone = without(key, make, rows)
    np.testing.assert_array_equal(bits(ref), bits(alone), err_msg="the statement itself")
    assert np.all(np.isposinf(ref[rows]))
    for name, o in orders(pts).items():
        got = run(backend, pts, o)
        bad = np.flatnonzero(bits(got) != bits(alone))
        assert bad.size == 0, (f"order {name}: {bad.size} of {len(pts)} rows differ, first {bad[:5]}: "
                               f"got {got[bad[:5]]}, want {alone[bad[:5]]}")
    return pts, ref


@pytest.mark.parametrize("row", [0, 150, 299])
@pytest.mark.parametrize("axis", [0, 2])
def test_one_nan_coordinate_changes_no_other_row_under_any_order(backend, row, axis):
    def make():                                                  # P = 300: one full group and a partial one
        p = uniform(300, 21)
        p[row, axis] = np.nan
        return p
    pts, ref = check_bad_rows(backend, ("one_nan", row, axis), make, [row])
    ok = np.arange(300) != row
    assert np.all(np.isfinite(ref[ok])) and np.all(ref[ok] < 12.0) and np.all(ref[ok] > 0)


def nan_group():
    p = uniform(1300, 22)
    p[256:512] = np.nan
    p[600, 1] = np.nan                                           # and a lone one in a group that has a box
    return p


def test_a_whole_group_of_nan_rows(backend):
    rows = np.r_[256:512, 600]
    pts, ref = check_bad_rows(backend, "nan_group", nan_group, rows)
    ok = np.setdiff1d(np.arange(1300), rows)
    assert np.all(np.isfinite(ref[ok])) and np.all(ref[ok] < 12.0)


def test_nan_rows_stay_out_of_the_boxes(backend):
    """White box (knn_scratch_layout: records [P], boxes [2 * groups], super-boxes [2 * supers], 16 bytes each): the box of
    a group is that of its rows without a NaN coordinate, empty (+inf, -inf) when it has none.  A NaN row that entered a box
    in any form would not change a result; it would only stop the box from culling anything."""
    lib = backend.lib
    pts, ref = statement("nan_group", nan_group)
    P = len(pts)
    need = lib.gs2m_knn_scratch_bytes(P)
    assert need == 16 * (P + 2 * 6 + 2 * 1)
    scratch = backend.dev(np.zeros(need // 4, np.float32))
    out = backend.dev(np.zeros(P, np.float32))
    dp = backend.dev(pts)
    assert lib.gs2m_knn_mean_dist2(P, _ptr(dp), None, _ptr(scratch), need, _ptr(out), C.c_void_p(0)) == 0
    backend.sync()
    np.testing.assert_array_equal(bits(backend.host(out)), bits(ref))
    box = backend.host(scratch).reshape(-1, 4)[P:P + 12, :3].reshape(6, 2, 3)
    sbox = backend.host(scratch).reshape(-1, 4)[P + 12:P + 14, :3]
    for g in range(6):
        rows = pts[256 * g:256 * (g + 1)]
        rows = rows[~np.isnan(rows).any(axis=1)]
        if len(rows) == 0:
            assert np.all(np.isposinf(box[g, 0])) and np.all(np.isneginf(box[g, 1]))
        else:
            np.testing.assert_array_equal(box[g, 0], rows.min(axis=0))
            np.testing.assert_array_equal(box[g, 1], rows.max(axis=0))
    good = pts[~np.isnan(pts).any(axis=1)]
    np.testing.assert_array_equal(sbox[0], good.min(axis=0))
    np.testing.assert_array_equal(sbox[1], good.max(axis=0))


def test_small_clouds_with_nan(backend):
    def four():
        p = uniform(4, 23)
        p[2, 1] = np.nan
        return p
    pts, ref = check_bad_rows(backend, "four_one_nan", four, [2])
    ok = [0, 1, 3]
    d = knn_statement.mean_dist2(pts[ok])                        # P = 3: (d0 + d1 + FLT_MAX) / 3
    np.testing.assert_array_equal(bits(ref[ok]), bits(d))
    assert np.all(bits(ref[ok]) == bits(TWO_NEIGHBOURS)) and 1.134e38 < float(TWO_NEIGHBOURS) < 1.135e38

    def five():
        p = uniform(5, 24)
        p[np.arange(5), [0, 1, 2, 0, 1]] = np.nan
        p[4] = np.nan
        return p
    pts, ref = statement("five_all_nan", five)
    assert np.all(np.isposinf(ref))
    np.testing.assert_array_equal(bits(run(backend, pts)), bits(ref))


INF_CASES = {                                                    # (row, axis, value) ...
    "one_plus_inf": [(40, 0, np.inf)],
    "two_of_one_sign": [(40, 1, np.inf), (270, 1, np.inf)],      # inf - inf: a NaN d between the two
    "two_of_one_sign_in_one_wave": [(3, 2, -np.inf), (4, 2, -np.inf)],
    "plus_and_minus": [(0, 0, np.inf), (299, 0, -np.inf)],
    "inf_and_nan": [(10, 0, np.inf), (11, 0, np.nan), (12, 1, -np.inf)],
}


@pytest.mark.parametrize("name", sorted(INF_CASES))
def test_infinite_coordinates_change_no_other_row(backend, name):
    def make():
        p = uniform(300, 25)
        for row, axis, value in INF_CASES[name]:
            p[row, axis] = value
        return p
    rows = [row for row, _, _ in INF_CASES[name]]
    pts, ref = check_bad_rows(backend, ("inf", name), make, rows)
    ok = np.setdiff1d(np.arange(300), rows)
    assert np.all(np.isfinite(ref[ok])) and np.all(ref[ok] < 12.0)


FAR = np.float32(3e19)                                           # FAR * FAR = 9e38 > FLT_MAX: every distance to it overflows


@pytest.mark.parametrize("near,far", [(3, 1), (2, 2), (1, 3), (4, 1), (3, 2), (3, 3), (4, 2), (2, 4), (4, 3), (3, 4)])
def test_distances_that_overflow_count_as_missing(backend, near, far):
    """a tight cluster of `near` points and `far` points at +-3e19 on the axes, P = 4 .. 7: a far point is at "no distance"
    from everything, so it gets +inf, and a cluster point has near - 1 neighbours and is padded with FLT_MAX"""
    def make():
        c = (uniform(near, 26) * np.float32(0.01)).astype(np.float32)
        f = np.zeros((far, 3), np.float32)
        f[np.arange(far), np.arange(far) % 3] = np.where(np.arange(far) < 3, FAR, -FAR)
        return np.ascontiguousarray(np.concatenate([c, f])[np.random.default_rng(27).permutation(near + far)])
    pts, ref = statement(("overflow", near, far), make)
    assert 4 <= len(pts) <= 7
    got = run(backend, pts)
    np.testing.assert_array_equal(bits(got), bits(ref))
    np.testing.assert_array_equal(bits(run(backend, pts, np.arange(len(pts), dtype=np.int32)[::-1].copy())), bits(ref))
    is_far = np.abs(pts).max(axis=1) > 1
    assert is_far.sum() == far and np.all(np.isposinf(got[is_far]))
    if near >= 4:
        assert np.all(got[~is_far] < 1e-3)
    elif near == 3:
        assert np.all(bits(got[~is_far]) == bits(TWO_NEIGHBOURS))                  # 1.1342e38, not +inf
    else:
        assert np.all(np.isposinf(got[~is_far]))                                    # (d0 + FLT_MAX) + FLT_MAX overflows


def test_subnormal_distances_are_not_flushed(backend):
    def make():                                                  # integer multiples of 1e-23: d = n * 1e-46, f32's least is 1.4e-45
        k = np.random.default_rng(28).integers(0, 40, (200, 3))
        return (k * 1e-23).astype(np.float32)
    pts, ref = statement("subnormal", make)
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert np.all(ref < tiny) and (ref > 0).sum() > 100 and len(np.unique(ref)) > 3
    for name, o in orders(pts).items():
        np.testing.assert_array_equal(bits(run(backend, pts, o)), bits(ref), err_msg=name)


@pytest.mark.parametrize("P", [64, 65, 4096])                    # one wave, one wave and a lane, exactly one full super-box
def test_shapes_at_the_wave_and_the_super_box(backend, P):
    pts, ref = statement(("uniform", P), lambda: uniform(P, 3000 + P))
    for name, o in (("none", None), ("morton", morton_order(pts))):
        got = run(backend, pts, o)
        assert got.shape == (P,)
        np.testing.assert_array_equal(bits(got), bits(ref), err_msg=name)
    assert np.all(ref < 12.0) and np.all(ref > 0)
