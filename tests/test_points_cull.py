"""gs2m_points_cull_views (gs2mesh_amd/csrc/points_cull_kernels.h) on both back-ends: exactly equal to statement (a) of
tests/cull_statement.py (the header's f32 arithmetic in numpy + torch's own grid_sample), and equal to statement (b) (the
reference's lines with torch's matmul) wherever no pixel coordinate lies within tau of a rounding boundary."""
import ctypes as C

import numpy as np
import pytest

import cull_scene
import cull_statement
import dilate_statement
from gs2mesh_amd import evaluation
from gs2mesh_amd.rasterizer import _ptr

MASK = (130, 70)                     # (W, H) of every mask here
NORMS = [(130, 70), (1600, 1200)]    # the reference normalises by its image size, grid_sample scales by the mask's own
# max |t_(a) - t_f64| over the 1000 points x 3 views of `scene`, t = the mask-grid coordinate grid_sample rounds: measured
# 1.86e-5 at norm 130 x 70 and 1.83e-5 at 1600 x 1200 (test_against_the_reference_lines re-measures it).  Statement (b) sums
# in the BLAS's order, which is not ours to fix: a factor 4 on top.
MEASURED_ERR = 1.9e-5
TAU = 4 * MEASURED_ERR               # 7.6e-5 of a mask pixel, the tolerance line of include/gs2mesh_amd.h
_REF = {}
f32 = np.float32


def scene(norm):
    """1000 random points in front of three cameras that look at the object's centre, disc masks; computed once, never
    modified -> dict(points, proj [3,3,4], masks [3,H,W] 0 / 1, bits [3,H,nw], world, scale)"""
    if norm not in _REF:
        cams, _ = cull_scene.cameras(3, norm)
        proj, _ = evaluation.dtu_projections(cams)
        masks = (cull_scene.disc_masks(3, MASK) != 0).astype(np.uint8)
        _REF[norm] = dict(points=cull_scene.points(1000, 1), proj=proj, masks=masks, bits=dilate_statement.pack(masks != 0),
                          world=[cams[f"world_mat_{i}"] for i in range(3)], scale=[cams[f"scale_mat_{i}"] for i in range(3)])
        _REF[norm]["keep_a"] = {n: cull_statement.keep_a(_REF[norm]["points"], proj[:n], masks[:n], norm) for n in (0, 1, 3)}
    return _REF[norm]


def run(backend, points, proj, bits, norm, mask_size=MASK, fill=7):
    lib = backend.lib
    points = np.ascontiguousarray(points, f32).reshape(-1, 3)
    V, n = len(points), len(proj)
    dp, dm = backend.dev(points), backend.dev(np.ascontiguousarray(proj, f32).reshape(-1, 12))
    db = backend.dev(np.ascontiguousarray(bits).view(np.int64))
    keep = backend.dev(np.full(V + 3, fill, np.uint8))
    rc = lib.gs2m_points_cull_views(V, _ptr(dp), n, _ptr(dm), _ptr(db), mask_size[0], mask_size[1], float(norm[0]), float(norm[1]),
                                    _ptr(keep), C.c_void_p(0))
    assert rc == 0, lib.gs2m_last_error()
    backend.sync()
    out = backend.host(keep)
    assert np.all(out[V:] == fill)                                   # nothing behind keep[V] is written
    return out[:V]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("n_views", [0, 1, 3])
@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 1000])
def test_random_points_equal_statement_a(backend, V, n_views, norm):
    s = scene(norm)
    got = run(backend, s["points"][:V], s["proj"][:n_views], s["bits"][:n_views], norm)
    want = s["keep_a"][n_views][:V]
    np.testing.assert_array_equal(got, want.astype(np.uint8))
    if n_views == 0:
        assert np.all(got == 1)
    if V == 1000 and n_views == 3:
        assert 50 < want.sum() < 950                                 # the scene culls some and keeps some


# ---- hand-placed points: a camera whose arithmetic can be inverted exactly ---------------------------------------------------
# u = x / (z + 1e-6f), v = y / (z + 1e-6f); at Z the denominator is exactly 2
HAND_PROJ = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]], f32)
Z = f32(2) - f32(1e-6)
assert f32(Z + f32(1e-6)) == f32(2)


def grid_coord(value, axis, norm):
    """statement (a)'s mask-grid coordinate t of a point whose coordinate on ``axis`` is ``value`` (the other one mid-image)"""
    p = np.array([[value, 70.0, Z]], f32) if axis == 0 else np.array([[130.0, value, Z]], f32)
    return cull_statement.unnormalized(p, HAND_PROJ[0], norm, MASK)[2 + axis][0]


def place(target, axis, norm):
    """the f32 coordinate whose t is exactly ``target``: the f64 inverse of the projection, then the neighbouring floats"""
    x = f32(2.0 * target * (norm[axis] - 1) / (MASK[axis] - 1))
    lo = hi = x
    for _ in range(400):
        for c in (lo, hi):
            if grid_coord(c, axis, norm) == f32(target):
                return c
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
    raise AssertionError(f"no float lands on t = {target} exactly (axis {axis}, norm {norm})")


def beside(c, sign, axis, norm, what):
    """a float next to ``c`` on the ``sign`` side at which statement (a)'s g (``what`` = 0) or t (``what`` = 2) has moved"""
    def val(v):
        p = np.array([[v, v, Z]], f32)
        return cull_statement.unnormalized(p, HAND_PROJ[0], norm, MASK)[what + axis][0]
    base, d = val(c), f32(c)
    for _ in range(200):
        d = f32(sign * 1e-30) if d == 0 else (f32(d * 2) if c == 0 else np.nextafter(d, f32(sign * np.inf)))
        if val(d) != base:
            assert (val(d) > base) == (sign > 0)
            return d
    raise AssertionError(f"nothing moves next to {c}")


def hand_points(norm):
    """-> (points [V,3] f32, labels): along x against masks of column stripes, along y against row stripes"""
    pts, labels = [], []
    for axis, last in ((0, MASK[0] - 1), (1, MASK[1] - 1)):
        def add(value, label):
            pts.append([value, 2.0 * 35 * (norm[1] - 1) / (MASK[1] - 1), Z] if axis == 0 else [2.0 * 64 * (norm[0] - 1) / (MASK[0] - 1), value, Z])
            labels.append((axis, label))
        # integers and ties of both parities.  Not every t is the image of a float (t = 10 is not: its neighbours give
        # 9.999997 and 10.000001), so each kind takes the first t of its list that is
        for kind, first in (("even", 32.0), ("odd", 33.0), ("tie above even", 32.5), ("tie above odd", 33.5)):
            c = None
            for t in (first, first + 2, first - 2, first + 4, first - 4, first + 6, first - 6):
                try:
                    c = place(t, axis, norm)
                    break
                except AssertionError:
                    continue
            assert c is not None, (kind, axis, norm)
            add(c, kind)
            add(beside(c, -1, axis, norm, 2), kind + "-")
            add(beside(c, +1, axis, norm, 2), kind + "+")
        for t, name in ((0.0, "g=-1"), (float(last), "g=+1")):                 # exactly on the open interval's ends,
            c = place(t, axis, norm)                                           # just inside and just outside them
            g = cull_statement.unnormalized(np.array([[c, c, Z]], f32), HAND_PROJ[0], norm, MASK)[axis][0]
            assert g == (f32(-1) if t == 0 else f32(1))
            add(c, name)
            add(beside(c, -1, axis, norm, 0), name + "-")
            add(beside(c, +1, axis, norm, 0), name + "+")
        for t in (-0.5, float(last) + 0.5, -1.0, float(last) + 1.0, -0.49, float(last) + 0.49):   # around the image's edge
            add(f32(2.0 * t * (norm[axis] - 1) / (MASK[axis] - 1)), f"edge t={t}")
    mid = [2.0 * 64 * (norm[0] - 1) / (MASK[0] - 1), 2.0 * 35 * (norm[1] - 1) / (MASK[1] - 1)]
    zero_den = -f32(1e-6)
    assert f32(zero_den + f32(1e-6)) == 0
    special = [([-mid[0], -mid[1], -Z], "behind the camera"), ([-mid[0] - 2, -mid[1], -2.5], "behind the camera, odd column"),
               ([0, 0, zero_den], "0 / 0"), ([1, 1, zero_den], "+inf"), ([-1, 1, zero_den], "-inf, +inf"), ([1, -1, zero_den], "+inf, -inf"),
               ([np.nan, mid[1], Z], "x NaN"), ([mid[0], np.nan, Z], "y NaN"), ([mid[0], mid[1], np.nan], "z NaN"),
               ([np.inf, mid[1], Z], "x +inf"), ([-np.inf, mid[1], Z], "x -inf"), ([mid[0], np.inf, Z], "y +inf"),
               ([mid[0], -np.inf, Z], "y -inf"), ([mid[0], mid[1], np.inf], "z +inf"), ([mid[0], mid[1], -np.inf], "z -inf"),
               ([np.inf, np.inf, np.inf], "all +inf"), ([mid[0], mid[1], Z], "mid-image")]
    for p, label in special:
        pts.append(p)
        labels.append((2, label))
    return np.asarray(pts, f32), labels


def stripes(axis, parity):
    y, x = np.mgrid[0:MASK[1], 0:MASK[0]]
    return (((x if axis == 0 else y) % 2) == parity).astype(np.uint8)


@pytest.mark.parametrize("norm", NORMS)
def test_hand_placed_points_equal_statement_a(backend, norm):
    key = ("hand", norm)
    if key not in _REF:
        pts, labels = hand_points(norm)
        masks = {(a, p): stripes(a, p)[None] for a in (0, 1) for p in (0, 1)}
        _REF[key] = (pts, labels, masks, {k: cull_statement.keep_a(pts, HAND_PROJ, m, norm) for k, m in masks.items()})
    pts, labels, masks, want = _REF[key]
    got = {k: run(backend, pts, HAND_PROJ, dilate_statement.pack(m != 0), norm) for k, m in masks.items()}
    for k in masks:
        np.testing.assert_array_equal(got[k], want[k].astype(np.uint8), err_msg=str(k))
    by = {lab: i for i, lab in enumerate(labels)}
    even_x, odd_x, even_y, odd_y = got[(0, 0)], got[(0, 1)], got[(1, 0)], got[(1, 1)]
    # integers land on their pixel; a tie goes to the even one, whichever side it is on, and the floats next to it to theirs
    for axis in (0, 1):
        even, odd = got[(axis, 0)], got[(axis, 1)]
        pick = lambda g, lab: int(g[by[(axis, lab)]])
        assert [pick(even, "even"), pick(odd, "even"), pick(even, "odd"), pick(odd, "odd")] == [1, 0, 0, 1]
        for tie in ("tie above even", "tie above odd"):
            assert pick(even, tie) == 1 and pick(odd, tie) == 0
        assert [pick(even, "tie above even-"), pick(even, "tie above even+")] == [1, 0]
        assert [pick(even, "tie above odd-"), pick(even, "tie above odd+")] == [0, 1]
    even_x, odd_x = got[(0, 0)], got[(0, 1)]
    # on g = +-1 and beyond it the view passes whatever the mask holds; just inside the mask decides (pixel 0 / the last)
    for axis, last in ((0, MASK[0] - 1), (1, MASK[1] - 1)):
        for parity in (0, 1):
            g = got[(axis, parity)]
            assert g[by[(axis, "g=-1")]] == 1 and g[by[(axis, "g=-1-")]] == 1 and g[by[(axis, "g=+1")]] == 1 and g[by[(axis, "g=+1+")]] == 1
            assert g[by[(axis, "g=-1+")]] == (1 if parity == 0 else 0)
            assert g[by[(axis, "g=+1-")]] == (1 if last % 2 == parity else 0)
            assert g[by[(axis, "edge t=-1.0")]] == 1 and g[by[(axis, f"edge t={last + 1.0}")]] == 1
    # NaN, infinities and a zero denominator: never valid, never sampled, so every such point passes
    for lab, i in by.items():
        if lab[0] == 2 and lab[1] not in ("mid-image", "behind the camera", "behind the camera, odd column"):
            assert all(g[i] == 1 for g in got.values()), lab
    # a point behind the camera goes through the same formula: (-x, -y, -z) lands where (x, y, z) does
    assert even_x[by[(2, "behind the camera")]] == even_x[by[(2, "mid-image")]] == 1
    assert odd_x[by[(2, "behind the camera")]] == 0


def test_a_point_that_fails_in_one_view_only(backend):
    norm = MASK
    full, even = np.ones((MASK[1], MASK[0]), np.uint8), stripes(0, 0)
    y = 2.0 * 35
    pts = np.array([[2.0 * 11, y, Z], [2.0 * 10, y, Z]], f32)        # pixel 11: off the even stripes; pixel 10: on them
    proj = np.repeat(HAND_PROJ, 3, axis=0)
    for masks in ([full, full, even], [even, full, full], [full, even, full]):
        m = np.stack(masks)
        got = run(backend, pts, proj, dilate_statement.pack(m != 0), norm)
        np.testing.assert_array_equal(got, cull_statement.keep_a(pts, proj, m, norm).astype(np.uint8))
        assert list(got) == [0, 1]
    got = run(backend, pts, proj, dilate_statement.pack(np.stack([full, full, full]) != 0), norm)
    assert list(got) == [1, 1]


def test_two_runs_give_equal_bytes(backend):
    s = scene(NORMS[1])
    a = run(backend, s["points"], s["proj"], s["bits"], NORMS[1], fill=0)
    b = run(backend, s["points"], s["proj"], s["bits"], NORMS[1], fill=255)
    np.testing.assert_array_equal(a, b)
    assert set(np.unique(a)) <= {0, 1}


@pytest.mark.parametrize("norm", NORMS)
def test_against_the_reference_lines(backend, norm):
    """statement (b): a keep-bit may differ only where some view's exact pixel coordinate is within TAU of a half-integer or
    of an image bound -- and the scene is chosen so that at most 5 % of it is that close"""
    s = scene(norm)
    key = ("b", norm)
    if key not in _REF:
        tx, ty = cull_statement.exact_pixels(s["points"], s["world"], s["scale"], norm, MASK)
        err = 0.0
        for i in range(3):
            _, _, ax, ay = cull_statement.unnormalized(s["points"], s["proj"][i], norm, MASK)
            err = max(err, float(np.abs(ax - tx[i]).max()), float(np.abs(ay - ty[i]).max()))

        def near(t, size):
            return (np.abs((t - 0.5) - np.round(t - 0.5)) <= TAU) | (np.abs(t) <= TAU) | (np.abs(t - (size - 1)) <= TAU)
        _REF[key] = (cull_statement.keep_b(s["points"], s["world"], s["scale"], s["masks"], norm), err,
                     (near(tx, MASK[0]) | near(ty, MASK[1])).any(axis=0))
    keep_b, err, close = _REF[key]
    print(f"norm {norm}: max |t_a - t_f64| = {err:.3e} (MEASURED_ERR {MEASURED_ERR}), tau = {TAU}, {close.sum()} of 1000 within tau")
    assert err <= MEASURED_ERR
    assert close.mean() <= 0.05
    got = run(backend, s["points"], s["proj"], s["bits"], norm).astype(bool)
    differ = got != keep_b
    assert np.all(close[differ]), np.nonzero(differ & ~close)
    assert np.all((s["keep_a"][3] != keep_b) <= close)               # the condition on the scene, statement against statement


def test_arguments(backend):
    lib = backend.lib
    s = scene(NORMS[0])
    dp, dm = backend.dev(s["points"]), backend.dev(s["proj"].reshape(-1, 12))
    db = backend.dev(s["bits"].view(np.int64))
    keep = backend.dev(np.full(1000, 7, np.uint8))
    st = C.c_void_p(0)

    def call(V=1000, p=dp, n=3, m=dm, b=db, w=MASK[0], h=MASK[1], k=keep):
        return lib.gs2m_points_cull_views(V, _ptr(p), n, _ptr(m), _ptr(b), w, h, 130.0, 70.0, _ptr(k), st)

    for bad, word in ((dict(V=-1), "V = -1"), (dict(n=-1), "n_views = -1"), (dict(p=None), "NULL points"), (dict(k=None), "NULL points or keep"),
                      (dict(m=None), "NULL proj"), (dict(b=None), "NULL proj or mask_bits"), (dict(w=0), "0 x 70"), (dict(h=0), "130 x 0")):
        assert call(**bad) == 1, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert call(V=0) == 0 and call(V=0, p=None, m=None, b=None, k=None) == 0
    backend.sync()
    assert np.all(backend.host(keep) == 7)                           # refused calls and V = 0 write nothing
    assert call(n=0, m=None, b=None, w=0, h=0) == 0                  # no views: nothing else is looked at
    backend.sync()
    assert np.all(backend.host(keep) == 1)
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(backend.host(keep), s["keep_a"][3].astype(np.uint8))


def test_cull_points_wrapper(backend):
    s = scene(NORMS[1])
    keep = evaluation.cull_points(backend.dev(s["points"]), s["proj"], backend.dev(s["bits"].view(np.int64)), MASK, NORMS[1],
                                  lib=backend.lib)
    backend.sync()
    got = keep.detach().cpu().numpy()
    assert got.dtype == bool
    np.testing.assert_array_equal(got, s["keep_a"][3])
    with pytest.raises(ValueError, match="mask_bits"):
        evaluation.cull_points(backend.dev(s["points"]), s["proj"], backend.dev(s["bits"][:2].view(np.int64)), MASK, lib=backend.lib)
