"""What the cross-view filter is for, measured on the numpy statement of its vote (tests/consistency_statement.py; the kernel
equals it bit for bit, tests/test_depth_consistency.py): on the ring scene with 5 % injected outliers (0.7-0.95 x and
1.05-1.3 x the true depth) it removes the outliers and keeps the surface.  CPU only.

Measured with this statement (ring of 12, 96 x 64, sources i+-1, i+-2, rel_tol 0.01); every bar leaves a margin below it:
    (min_support 2, max_violation 1)   outliers removed 0.9968 of 1231    inliers kept 0.9552 of 24509
    (2, 0)                             outliers removed 0.9968            inliers kept 0.8306
    noise-free, (2, 1)                 valid pixels kept 0.9879
Also here: select_sources and pair_matrices on that ring."""
import numpy as np
import pytest

import consistency_statement as cs
from gs2mesh_amd.depth_utils import ConsistencyParams, pair_matrices, select_sources


@pytest.fixture(scope="module")
def ring():
    s = cs.ring_scene()
    g = cs.RING
    s["votes"] = cs.votes(s["depths"], s["intrinsics"], s["sources"], s["pair"], g["rel_tol"], g["min_depth"], g["max_depth"])
    return s


def rates(scene, min_support, max_violation):
    valid, sup, vio, _ = scene["votes"]
    keep = cs.keep_maps(valid, sup, vio, min_support, max_violation)
    out = np.stack(scene["outlier"])
    inl = np.stack([(d > 0) & ~m for d, m in zip(scene["clean"], scene["outlier"])])
    keep = np.stack(keep).astype(bool)
    return int(out.sum()), float((~keep[out]).mean()), int(inl.sum()), float(keep[inl].mean())


def test_outliers_go_and_inliers_stay(ring):
    n_out, removed, n_in, kept = rates(ring, 2, 1)
    print(f"(2, 1): {n_out} outliers, removed {removed:.4f}; {n_in} inliers, kept {kept:.4f}")
    assert (n_out, n_in) == (1231, 24509)
    assert removed >= 0.99
    assert kept >= 0.93


def test_no_violation_allowed(ring):
    _, removed, _, kept = rates(ring, 2, 0)
    print(f"(2, 0): removed {removed:.4f}, kept {kept:.4f}")
    assert removed >= 0.99
    assert kept >= 0.80


def test_noise_free_scene_keeps_its_surface():
    s = cs.ring_scene(noise=False)
    g = cs.RING
    keep, *_ = cs.consistency(s["depths"], s["intrinsics"], s["sources"], s["pair"], g["rel_tol"], g["min_depth"],
                              g["max_depth"], 2, 1)
    valid = np.stack(s["clean"]) > 0
    kept = float(np.stack(keep).astype(bool)[valid].mean())
    print(f"noise-free (2, 1): kept {kept:.4f} of {int(valid.sum())}")
    assert not np.stack(keep).astype(bool)[~valid].any()
    assert kept >= 0.97


def test_select_sources_on_the_ring(ring):
    n = cs.RING["n"]
    got = select_sources(ring["camera_to_world"], k=4, max_angle_deg=70.0)
    assert got.dtype == np.int32 and got.shape == (n, 4)
    for i in range(n):
        near, far = sorted([(i - 1) % n, (i + 1) % n]), sorted([(i - 2) % n, (i + 2) % n])
        assert got[i].tolist() == near + far, i                  # nearest first, the lower index first within a tie
    # the angle bound: 30 degrees between neighbours, so 45 admits i+-1 only; the rest is -1 padding
    got = select_sources(ring["camera_to_world"], k=3, max_angle_deg=45.0)
    for i in range(n):
        assert got[i].tolist() == sorted([(i - 1) % n, (i + 1) % n]) + [-1], i
    assert select_sources(ring["camera_to_world"][:1], k=2).tolist() == [[-1, -1]]
    assert select_sources(ring["camera_to_world"], k=0).shape == (n, 0)
    with pytest.raises(ValueError):
        select_sources(ring["camera_to_world"], k=17)


def test_pair_matrices(ring):
    E = ring["camera_to_world"]
    src = np.array(ring["sources"])
    src[3, 1] = -1
    P = pair_matrices(E, src)
    assert P.dtype == np.float32 and P.shape == (len(E), 4, 12)
    for i in range(len(E)):
        for k, j in enumerate(src[i]):
            want = (np.linalg.inv(E[j]) @ E[i])[:3].astype(np.float32).reshape(12) if j >= 0 else np.zeros(12, np.float32)
            assert np.array_equal(P[i, k], want), (i, k)
    # the same thing as world -> camera of j after camera -> world of i
    w2c = np.concatenate([ring["poses"], np.tile([[[0, 0, 0, 1.0]]], (len(E), 1, 1))], axis=1)
    np.testing.assert_allclose(P[0, 0].reshape(3, 4), (w2c[src[0, 0]] @ E[0])[:3], atol=1e-6)


def test_params_coerce():
    assert ConsistencyParams.coerce(None) is None and ConsistencyParams.coerce(False) is None
    assert ConsistencyParams.coerce(True) == ConsistencyParams(4, 0.01, 2, 1, 70.0)
    assert ConsistencyParams.coerce(dict(rel_tol=0.02, sources=6)) == ConsistencyParams(sources=6, rel_tol=0.02)
    p = ConsistencyParams(min_support=3)
    assert ConsistencyParams.coerce(p) is p
    with pytest.raises(TypeError):
        ConsistencyParams.coerce(4)
