"""gs2mesh_amd.evaluation's registration on both back-ends: ``umeyama`` on known transforms, ``registration_icp`` on a sphere patch
against the perturbation it was given, against the same loop driven by the numpy statement of the kernel (bit for bit) and
against an independent float64 KD-tree ICP, and MobileBrick's alignment rule."""
import numpy as np
import pytest

import icp_statement
from gs2mesh_amd import evaluation
from gs2mesh_amd.mesh import TriangleMesh

_REF = {}


def rigid(angle, axis, t, scale=1.0):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K))
    T[:3, 3] = t
    return T


def apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def sphere_patch(n=2000, radius=2.0, cap=0.6, centre=(0.3, -0.2, 0.5)):
    """n points spread evenly (a Fibonacci spiral) over the cap of half-angle `cap` of a sphere: spacing about
    radius * sqrt(2 pi (1 - cos cap) / n) = 0.047 for the defaults"""
    i = np.arange(n) + 0.5
    z = 1 - (1 - np.cos(cap)) * i / n
    phi = i * np.pi * (3 - np.sqrt(5))
    r = np.sqrt(1 - z * z)
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) + np.asarray(centre)


PERTURBATIONS = {"rigid": (rigid(0.003, (1, -2, 0.5), (0.004, -0.003, 0.002)), False),
                 "similarity": (rigid(0.003, (1, -2, 0.5), (0.004, -0.003, 0.002), scale=1.003), True)}
MAX_DIST = 0.1


def case(name):
    """source, target = P(source), origin: the displacement (at most 0.003 * 2.6 + 0.0054 + 0.003 * 2.6 of scale = 0.021, 0.013 when rigid) is below half the spacing, so the first pairs are
    mostly the true ones and the loop ends on all of them"""
    P, scaling = PERTURBATIONS[name]
    s = sphere_patch()
    t = apply(P, s)
    return s, t, (t.min(0) + t.max(0)) / 2, P, scaling


# ---- umeyama ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_umeyama_recovers_a_known_transform(scale):
    rng = np.random.default_rng(0)
    s = rng.normal(0, 1, (200, 3)) * [3, 1, 0.5] + [10, -4, 2]
    T = rigid(0.8, (0.2, 1, -0.5), (1.5, -2.5, 0.7), scale)
    got = evaluation.umeyama(s, apply(T, s), with_scaling=scale != 1.0)
    np.testing.assert_allclose(got, T, rtol=0, atol=1e-12)           # rounding of an exact fit: a few hundred ulps of O(10) values
    assert np.array_equal(got[3], [0, 0, 0, 1])
    if scale != 1.0:                                                  # without scaling the rotation is the same, c stays 1
        R = evaluation.umeyama(s, apply(T, s), with_scaling=False)[:3, :3]
        np.testing.assert_allclose(R, T[:3, :3] / scale, rtol=0, atol=1e-12)
    # the moments of the kernel give the same transform: here from an origin inside the cloud
    o = np.array([9.0, -4.5, 2.5])
    a, b = s - o, apply(T, s) - o
    m = evaluation.umeyama_from_moments(len(s), a.sum(0), b.sum(0), a.T @ b, (a * a).sum(), o, with_scaling=scale != 1.0)
    np.testing.assert_allclose(m, T, rtol=0, atol=1e-11)


def test_umeyama_gives_a_proper_rotation_on_mirrored_input():
    rng = np.random.default_rng(1)
    s = rng.normal(0, 1, (300, 3)) * [2, 1, 0.3]
    d = s * [1, 1, -1]                                                # the best orthogonal map is a reflection
    for scaling in (False, True):
        T = evaluation.umeyama(s, d, with_scaling=scaling)
        c = np.cbrt(np.linalg.det(T[:3, :3]))
        assert c > 0
        np.testing.assert_allclose(np.linalg.det(T[:3, :3] / c), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose((T[:3, :3] / c) @ (T[:3, :3] / c).T, np.eye(3), rtol=0, atol=1e-12)


def test_umeyama_of_no_pairs_is_the_identity():
    assert np.array_equal(evaluation.umeyama(np.zeros((0, 3)), np.zeros((0, 3)), True), np.eye(4))
    assert np.array_equal(evaluation.umeyama_from_moments(0, np.zeros(3), np.zeros(3), np.zeros((3, 3)), 0.0, (1, 2, 3)), np.eye(4))
    with pytest.raises(ValueError):
        evaluation.umeyama(np.zeros((2, 3)), np.zeros((3, 3)))


# ---- registration_icp ------------------------------------------------------------------------------------------------------

def run_icp(backend, name, **kw):
    s, t, o, P, scaling = case(name)
    return evaluation.registration_icp(backend.dev(s), backend.dev(t), MAX_DIST, with_scaling=scaling, origin=o, lib=backend.lib, **kw)


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
def test_icp_converges_to_the_perturbation_and_stops_early(backend, name):
    """Once every pair is a true pair the update is the exact least-squares fit of an exact transform, so what is left is
    rounding: f64 sums of 2000 O(1) terms and their raw-moment cancellation, far below 1e-9."""
    P = PERTURBATIONS[name][0]
    r = run_icp(backend, name, want_correspondences=True)
    print(f"max|T - P| = {np.abs(r.transformation - P).max():.3e}, rmse = {r.inlier_rmse:.3e}, iterations = {r.n_iterations}")
    assert r.fitness == 1.0 and 1 <= r.n_iterations < 30             # the relative criteria ended it, not max_iteration
    assert np.abs(r.transformation - P).max() < 1e-9 and r.inlier_rmse < 1e-9
    np.testing.assert_array_equal(r.correspondence_set, np.stack([np.arange(2000), np.arange(2000)], 1))
    assert run_icp(backend, name, max_iteration=1).n_iterations == 1
    zero = run_icp(backend, name, max_iteration=0)
    assert zero.n_iterations == 0 and np.array_equal(zero.transformation, np.eye(4)) and 0 < zero.inlier_rmse < 0.02


def statement_loop(name):
    """icp_loop driven by the numpy statement of the kernel: computed once, shared between the back-ends"""
    if name not in _REF:
        s, t, o, P, scaling = case(name)

        def step(T):
            ref = icp_statement.icp_step(s, T, t, o, MAX_DIST)
            return ref["n"], ref["sums"]
        _REF[name] = evaluation.icp_loop(step, len(s), None, scaling, origin=o)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
@pytest.mark.parametrize("sort", [True, False])
def test_icp_equals_the_loop_on_the_statement_bit_for_bit(backend, name, sort):
    T, fitness, rmse, done = statement_loop(name)
    r = run_icp(backend, name, sort=sort)
    np.testing.assert_array_equal(r.transformation.view(np.uint64), T.view(np.uint64))
    assert (r.fitness, r.inlier_rmse, r.n_iterations) == (fitness, rmse, done)


def centred_umeyama(s, d, scaling):
    n = len(s)
    if n == 0:
        return np.eye(4)
    ms, md = s.mean(0), d.mean(0)
    U, D, Vt = np.linalg.svd((d - md).T @ (s - ms) / n)
    S = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / ((s - ms) ** 2).sum() * n if scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * R @ ms
    return T


def kd_tree_icp(s, t, max_dist, scaling, max_iteration=30, rel=1e-6):
    """Open3D's loop in float64 on a KD tree, transforming the points in place by every update as Open3D does"""
    from scipy.spatial import cKDTree
    tree = cKDTree(t)
    T, p = np.eye(4), s.copy()

    def evaluate(p):
        d, j = tree.query(p)
        k = d < max_dist
        return k, j, k.sum() / len(p), (np.sqrt((d[k] ** 2).mean()) if k.any() else 0.0)

    k, j, fit, rmse = evaluate(p)
    for _ in range(max_iteration):
        U = centred_umeyama(p[k], t[j[k]], scaling)
        T, p = U @ T, apply(U, p)
        before = (fit, rmse)
        k, j, fit, rmse = evaluate(p)
        if abs(before[0] - fit) < rel and abs(before[1] - rmse) < rel:
            break
    return T


# max|T - T_ref| of the two named cases, measured on the emulator build (the GPU build gives the emulator's bits, by the test above)
MEASURED_KD_DIFFERENCE = {"rigid": 1.331e-15, "similarity": 5.274e-16}


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
def test_icp_against_an_independent_float64_kd_tree_icp(backend, name):
    """The bound is 8 x the measured difference: the margin is for another neighbour at an f32 near-tie, for raw against
    centred moments, and for Open3D's in-place transform against the accumulated one."""
    s, t, o, P, scaling = case(name)
    if ("kd", name) not in _REF:
        _REF[("kd", name)] = kd_tree_icp(s, t, MAX_DIST, scaling)
    diff = np.abs(run_icp(backend, name).transformation - _REF[("kd", name)]).max()
    print(f"{name}: max|T - T_ref| = {diff:.3e}")
    assert diff <= 8 * MEASURED_KD_DIFFERENCE[name]


# ---- MobileBrick's alignment -------------------------------------------------------------------------------------------------

def test_mobilebrick_align_applies_the_inverse_only_above_the_fitness(backend):
    gt_v = sphere_patch()
    tris = np.stack([np.arange(0, 1998), np.arange(1, 1999), np.arange(2, 2000)], 1).astype(np.int32)
    gt = TriangleMesh(gt_v, tris)
    P = PERTURBATIONS["rigid"][0]
    pred = TriangleMesh(apply(P, gt_v), tris)
    before = pred.vertices.copy()
    out, r = evaluation.mobilebrick_align(pred, gt, lib=backend.lib)
    assert r.fitness == 1.0 and r.n_iterations <= 10
    np.testing.assert_allclose(r.transformation, P, rtol=0, atol=1e-9)                    # GT -> prediction
    np.testing.assert_allclose(out.vertices, gt_v, rtol=0, atol=1e-8)                     # the prediction came back onto the GT
    assert np.array_equal(pred.vertices, before) and np.array_equal(out.triangles, tris)  # a copy: the input is untouched
    # a prediction that lacks 5 % of the GT region (the cap's outer rim: spacing 0.047 > threshold 0.02, so the GT
    # vertices there find nobody): fitness 0.95, the mesh stays where it is
    part = TriangleMesh(apply(P, gt_v[:1900]), tris[:1898])
    out, r = evaluation.mobilebrick_align(part, gt, lib=backend.lib)
    assert 0.94 < r.fitness <= 0.99
    assert np.array_equal(out.vertices, part.vertices) and out is not part
    # the threshold is a parameter: the same pair passes with a lower one
    out, r2 = evaluation.mobilebrick_align(part, gt, min_fitness=0.9, lib=backend.lib)
    assert r2.fitness == r.fitness
    np.testing.assert_allclose(out.vertices, gt_v[:1900], rtol=0, atol=1e-8)
