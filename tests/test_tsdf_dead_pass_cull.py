"""The dead-pass cull of the batch sweep (k_tsdf_integrate_batch + k_tsdf_depth_tiles): lane f of a wave tests frame f for the
wave's micro-column (4 x 4 x 16 voxels) against a max-depth map of 8 x 8-pixel tiles, and the wave walks only the frames the
test cannot prove dead.  A culled pass must be one that would have updated nothing, so every case asks what the other sweep
tests ask -- batch sweep == frame-by-frame calls == oracle, bit for bit, on the block set, tsdf, weight, the integer colour
sums and block_updates (``check_all_three`` of test_tsdf_sweep_layout.py) -- on scenes built to put the test's branches and
margins on the line.

What a scene is there for is asserted first, with ``probe`` of test_tsdf_edges.py (which voxels a frame updates) and the
restatement of the kernel's test in tools/tsdf_dead_pass_census.py (``proven_dead``: which passes the test culls, and by which
of its three reasons): a scene that culls nothing, or keeps nothing, fails instead of passing vacuously.  ``model`` also
asserts, for every scene, that no culled pass holds a voxel the frame updates.

Most scenes look at block (0, 0, 0) = [0, 0.25]^3 (voxel 1 / 64) along +y from 4 units away at 6 pixels per voxel: the waves of
a work item differ in their y-quarter, so a surface y = const cuts a work item into waves in front of, inside and behind the
band.  References are computed once per scene and shared between the back-ends.
"""
import os
import sys

import numpy as np
import pytest

from test_tsdf_edges import (ROTS, Scene, assert_same_volume, colours, extrinsic, integrate_batch, integrate_frames, probe, scene,
                             touched, volume)
from test_tsdf_sweep_layout import check_all_three

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from tsdf_dead_pass_census import column_updates, proven_dead, tile_map  # noqa: E402

VL = 1.0 / 64
TRUNC = 0.06
BLOCK = (0, 0, 0)
OFF, NO_DEPTH, BEHIND = 1, 2, 3                      # proven_dead's reasons
ALONG_Y = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # camera z = world y, camera x = world x
W = H = 128
F = 6 * 64 * 4.0                                     # 6 pixels per voxel at distance 4
K0 = (W, H, F, F, 64.3, 63.6)
CENTRE = (0.125, -4.0, 0.125)


def model(sc, k, keys=(BLOCK,)):
    """for the blocks ``keys`` (sorted) under frame k: pass updates a voxel [n, xq, yq], pass culled, the reason, tiles read"""
    keys = sorted(keys)
    upd = column_updates(probe(sc, k, keys)["upd"])[0]
    dead, why, ntiles = proven_dead(keys, tile_map(sc.converted(k)), sc.K, sc.frames[k][2], sc.voxel, sc.trunc)
    assert not (dead & upd).any(), "the test's restatement culls a pass that updates a voxel"
    return upd, dead, why, ntiles


def wall(y_s, window=None):
    """depth image of the plane y = y_s seen from CENTRE along +y, inside the pixel window (u0, u1, v0, v1) only"""
    d = np.zeros((H, W), np.float32)
    u0, u1, v0, v1 = window or (28, 100, 28, 100)
    d[v0:v1, u0:u1] = np.float32(y_s + 4.0)
    return d


def walls_scene(planes, color=True, key=None, **kw):
    def make():
        rng = np.random.default_rng(53)
        E = extrinsic(ALONG_Y, CENTRE)
        return Scene(K0, [(wall(y), colours(rng, W, H), E) for y in planes], VL, TRUNC, color=color, max_blocks=64, **kw)
    return scene(("cull-walls", tuple(planes), color, key), make)


# ---- 1. a work item with culled, live and idle waves; 6. the same without colour -------------------------------------------------
@pytest.mark.parametrize("color", [True, False])
def test_work_item_with_culled_live_and_idle_waves(backend, color):
    """Walls at y = 0.03, 0.09 and 0.03 again: waves 0 and 1 of every work item of block (0, 0, 0) are live in every frame, wave 2
    is behind the band of the first and third wall and inside the band of the second, wave 3 is behind every band and walks no
    frame at all (no state loads, no stores)."""
    sc = walls_scene((0.03, 0.09, 0.03), color)
    upd, dead, why = (np.stack(x) for x in zip(*(model(sc, k)[:3] for k in range(3))))       # [frame, 1, xq, yq]
    upd, dead, why = upd[:, 0], dead[:, 0], why[:, 0]
    assert all(BLOCK in touched(sc, k) for k in range(3))
    for xq in (1, 2):
        assert upd[:, xq, 0].all() and upd[:, xq, 1].all() and not dead[:, xq, :2].any()
        assert dead[:, xq, 2].tolist() == [True, False, True] and upd[1, xq, 2] and (why[[0, 2], xq, 2] == BEHIND).all()
        assert dead[:, xq, 3].all()
    print(f"mixed work item, colour {color}: culled passes per frame {dead.sum((1, 2)).tolist()} of 16, updating {upd.sum((1, 2)).tolist()}")
    check_all_three(backend, sc)


# ---- 2. the band's back edge, under a multiplier clearly above 1 -----------------------------------------------------------------
def back_edge_scene():
    """The camera looks along +y past the block, which sits 2.2 units to its right: (u - cx) / fx ~ 0.55, multiplier ~ 1.14.  The wall's
    depth is searched for (on the f32 model) so that in some micro-column of y-quarter 2 exactly ONE voxel is still updated."""
    def make():
        rng = np.random.default_rng(59)
        K = (W, H, F, F, 94.3 - 0.55 * F, 63.6)
        E = extrinsic(ALONG_Y, (0.125 - 2.2, -4.0, 0.125))
        col = colours(rng, W, H)

        def at(bits, lower=()):
            d = np.full((H, W), np.uint32(bits).view(np.float32), np.float32)
            for v, u in lower:
                d[v, u] = np.uint32(bits - 1).view(np.float32)
            sc = Scene(K, [(d, col, E)], VL, TRUNC, max_blocks=64)
            return sc, probe(sc, 0, [BLOCK])["upd"][0].reshape(4, 4, 4, 4, 16).sum((1, 3, 4))       # updating voxels per (xq, yq)

        lo, hi = (int(np.float32(x).view(np.uint32)) for x in (4.06, 4.10))         # bisection over the floats in between
        assert at(lo)[1][0, 2] == 0 and at(hi)[1][0, 2] > 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if at(mid)[1][0, 2] > 0 else (mid, hi)
        # hi: the least depth at which column (0, 2) updates a voxel.  One float of depth moves the sdf by more than neighbouring
        # voxels differ, so several may come in at once: all but one get a pixel of the depth just below
        p = probe(at(hi)[0], 0, [BLOCK])
        first = np.argwhere(p["upd"][0][:4, 8:12])
        return at(hi, [(int(p["v"][0][x, 8 + y, z]), int(p["u"][0][x, 8 + y, z])) for x, y, z in first[1:]])[0]
    return scene("cull-back-edge", make)


def test_band_back_edge_keeps_the_column_with_one_updating_voxel(backend):
    """A micro-column whose only updating voxel has its sdf just above -trunc is kept; its neighbour one y-quarter deeper, wholly
    below, is culled.  The pixel is far from the principal point, so the distance multiplier is clearly above 1: the test
    bounds (d - z) * mult by d - z only because mult >= 1."""
    sc = back_edge_scene()
    p = probe(sc, 0, [BLOCK])
    upd, dead, why, _ = model(sc, 0)
    n = p["upd"][0].reshape(4, 4, 4, 4, 16).sum((1, 3, 4))
    xq = int(np.flatnonzero(n[:, 2] == 1)[0])
    sdf = p["sample"][0][p["upd"][0] & (np.arange(16)[:, None, None] // 4 == xq) & (np.arange(16)[None, :, None] // 4 == 2)] * np.float32(TRUNC)
    u = p["u"][0][p["upd"][0]]
    mult = np.sqrt(1 + ((u - sc.K[4]) / sc.K[2]) ** 2).min()
    print(f"back edge: column (xq {xq}, yq 2) has one updating voxel, sdf + trunc = {float(sdf[0]) + TRUNC:.2e}; multiplier >= {mult:.3f}; "
          f"culled passes {int(dead.sum())} of 16")
    assert len(sdf) == 1 and 0 < float(sdf[0]) + TRUNC < 0.1 * VL and mult > 1.1
    assert upd[0, xq, 2] and not dead[0, xq, 2]
    assert dead[0, xq, 3] and why[0, xq, 3] == BEHIND and not upd[0, :, 3].any()
    # further right the footprints cover more than the 48 tiles the test is willing to read: those passes run untested
    assert (~dead[0, :, 3]).any()
    check_all_three(backend, sc)


# ---- 3. invalid samples next to a valid one; mask, min_depth, depth_trunc, depth_scale --------------------------------------------
VOXEL = (9, 6, 8)                                    # x-quarter 2, y-quarter 1: the voxel the special pixel is aimed at
VOXEL2 = (13, 6, 8)                                  # the same in x-quarter 3


def special_scene(kind):
    """x-quarter 0 of the block looks at a wall at y = 0.20 (live, and what touches the block); x-quarters 2 and 3 look at zero
    depth except for the pixel voxel VOXEL projects to, which holds a depth on that voxel (y = 0.1016) -- or does not, after the
    conversion the case is about."""
    def make():
        rng = np.random.default_rng(61)
        E = extrinsic(ALONG_Y, CENTRE)
        aim = Scene(K0, [(np.ones((H, W), np.float32), colours(rng, W, H), E)], VL, TRUNC)
        p = probe(aim, 0, [BLOCK])
        u, v = int(p["u"][0][VOXEL]), int(p["v"][0][VOXEL])
        u2, v2 = int(p["u"][0][VOXEL2]), int(p["v"][0][VOXEL2])
        assert 64 < u < 100 and 28 < v < 100 and (u % 8, v % 8) not in ((0, 0),)
        d = wall(0.20, (20, 40, 30, 100))
        hit = np.float32(4.0 + (VOXEL[1] + 0.5) * VL)
        kw, mask, scale = {}, None, 1.0
        d[v, u] = hit
        if kind == "invalid":                         # the tile of (u, v): NaN, +inf, a negative and zeros around the one valid pixel
            tv, tu = 8 * (v // 8), 8 * (u // 8)
            d[tv:tv + 8, tu:tu + 8] = np.array([np.nan, np.inf, -0.5, 0.0], np.float32)[np.arange(64).reshape(8, 8) % 4]
            d[v, u] = hit
        elif kind == "mask":                          # a second such pixel for x-quarter 3; the first one is masked out
            d[v2, u2] = hit
            mask = np.ones((H, W), np.uint8)
            mask[v, u] = 0
        elif kind == "min":
            kw = dict(min_depth=4.15)
        elif kind == "trunc":
            d[v, u] = np.float32(4.25)
            kw = dict(depth_trunc=4.22)
        elif kind == "scale":
            scale = 0.5
            kw = dict(depth_scale=0.5, depth_trunc=5.0)
        sc = Scene(K0, [((d * np.float32(scale)).astype(np.float32), colours(rng, W, H), E)], VL, TRUNC, masks=None if mask is None else [mask],
                   max_blocks=64, **kw)
        sc.pixel, sc.pixel2 = (u, v), (u2, v2)
        return sc
    return scene(("cull-special", kind), make)


@pytest.mark.parametrize("kind", ["invalid", "mask", "min", "trunc", "scale"])
def test_map_sees_the_depth_the_integrator_sees(backend, kind):
    """The map holds the CONVERTED depth: NaN, +inf, negative and zero samples in a tile do not hide (or poison) its one valid
    pixel; a pixel the mask, min_depth or depth_trunc removes is no sample (its footprints are culled as holding none); under
    depth_scale = 0.5 the raw values are half the depths the band test must compare."""
    sc = special_scene(kind)
    u, v = sc.pixel
    conv = sc.converted(0)
    upd, dead, why, _ = model(sc, 0)
    assert BLOCK in touched(sc, 0) and upd[0, 0].all() and not dead[0, 0].any()          # x-quarter 0: the wall
    xq, yq = VOXEL[0] // 4, VOXEL[1] // 4
    gone = kind in ("min", "trunc")
    if kind == "invalid":
        tile = conv[8 * (v // 8):8 * (v // 8) + 8, 8 * (u // 8):8 * (u // 8) + 8]
        with np.errstate(invalid="ignore"):
            assert np.isnan(tile).sum() >= 16 and (tile > 0).sum() == 1 and (sc.frames[0][0] == np.inf).any() and (sc.frames[0][0] < 0).any()
    if kind == "mask":
        u2, v2 = sc.pixel2
        assert conv[v, u] == 0 and conv[v2, u2] > 0 and sc.frames[0][0][v, u] > 0 and u // 8 != u2 // 8
        assert upd[0, 3].any() and (why[0, 2] == NO_DEPTH).all()
    elif gone:
        assert conv[v, u] == 0 and sc.frames[0][0][v, u] > 0 and not upd[0, 2:].any() and (why[0, 2:] == NO_DEPTH).all()
    else:
        if kind == "scale":
            assert sc.frames[0][0][v, u] < 2.1 and 4.0 < conv[v, u] < 4.2
        assert upd[0, xq, yq] and not dead[0, xq, yq] and probe(sc, 0, [BLOCK])["upd"][0][VOXEL]
        assert (why[0, xq + 1] == NO_DEPTH).all()
    print(f"special pixel ({kind}): culled passes {int(dead.sum())} of 16, by reason {np.bincount(why.ravel(), minlength=4)[1:].tolist()}")
    check_all_three(backend, sc)


# ---- 4. geometry limits ------------------------------------------------------------------------------------------------------
def limits_scene(Wi, Hi):
    """three cameras with roll inside the blocks they touch (test_tsdf_edges.inside_scene's recipe) on an image of Wi x Hi"""
    def make():
        rng = np.random.default_rng(100 * Wi + Hi)
        K = (Wi, Hi, 0.8 * Wi + 1.5, 1.1 * Hi + 0.7, 0.31 * Wi, 0.68 * Hi)
        ramp = np.linspace(0.03, 1.2, Wi * Hi).astype(np.float32)
        frames = []
        for k, R in enumerate(ROTS):
            d = (ramp.reshape(Hi, Wi), ramp[::-1].reshape(Hi, Wi), ramp.reshape(Wi, Hi).T)[k]
            frames.append((np.ascontiguousarray(d), colours(rng, Wi, Hi), extrinsic(R, (0.11 - 0.05 * k, -0.07, 0.05 + 0.03 * k))))
        return Scene(K, frames, 1.0 / 32, 0.06, max_blocks=768)
    return scene(("cull-limits", Wi, Hi), make)


@pytest.mark.parametrize("Wi,Hi", [(37, 29), (5, 3)])
def test_geometry_limits(backend, Wi, Hi):
    """Cameras inside the volume: micro-columns with a corner at or behind the camera plane (never culled), footprints wholly
    off the image (culled), partly off it (clipped), over several tiles of a 37 x 29 image (5 x 4 tiles, the last column and
    row partial), and an image smaller than one tile."""
    sc = limits_scene(Wi, Hi)
    fig = dict(behind=0, off=0, partly=0, straddle=0, culled=0, live=0)
    for k in range(len(sc.frames)):
        keys = sorted(touched(sc, k))
        p = probe(sc, k, keys)
        upd, dead, why, ntiles = model(sc, k, keys)
        col = lambda a, how: getattr(a.reshape(len(keys), 4, 4, 4, 4, 16), how)((2, 4, 5))
        some_behind = col(~p["front"], "any")
        assert not (dead & some_behind).any()                    # a voxel with z <= 0: the hull argument does not hold, live
        fig["behind"] += int(some_behind.sum())
        fig["off"] += int((why == OFF).sum())
        fig["partly"] += int((col(p["acc"], "any") & col(~p["acc"] & p["front"], "any") & ~dead).sum())
        fig["straddle"] += int((ntiles > 1).sum())
        fig["culled"] += int(dead.sum())
        fig["live"] += int((~dead).sum())
    print(f"limits {Wi}x{Hi}: {fig}")
    assert fig["behind"] > 0 and fig["off"] > 0 and fig["partly"] > 0 and fig["culled"] > 0 and fig["live"] > 0
    if Wi >= 8:
        assert fig["straddle"] > 0 and Wi % 8 and Hi % 8
    else:
        assert Wi < 8 and Hi < 8
    check_all_three(backend, sc)


# ---- 5. batch shapes ---------------------------------------------------------------------------------------------------------
def many_scene(n, size=64):
    """n frames of one camera along +y on a small image (3 pixels per voxel), the wall stepping through the block: every frame
    touches block (0, 0, 0) and culls another set of its waves"""
    def make():
        rng = np.random.default_rng(67 + n)
        f = 3 * 64 * 4.0 * size / 64
        K = (size, size, f, f, size / 2 + 0.3, size / 2 - 0.4)
        E = extrinsic(ALONG_Y, CENTRE)
        col = colours(rng, size, size)
        frames = []
        for k in range(n):
            d = np.zeros((size, size), np.float32)
            d[size // 4:3 * size // 4, size // 4:3 * size // 4] = np.float32(4.0 + 0.02 + 0.16 * ((7 * k) % 16) / 16)
            frames.append((d, col, E))
        return Scene(K, frames, VL, TRUNC, max_blocks=64)
    return scene(("cull-many", n, size), make)


@pytest.mark.parametrize("n", [1, 64, 70])
def test_batches_of_1_64_and_70_frames(backend, n):
    """One frame (one lane tests), 64 frames that all touch the block (every lane tests a frame), and 70 frames in one call: two
    sub-batches that use the same map buffer one after the other."""
    sc = many_scene(n)
    assert all(BLOCK in touched(sc, k) for k in range(n))
    dead = np.stack([model(sc, k)[1][0] for k in range(n)])
    print(f"batch of {n}: culled passes per frame, min .. max {int(dead.sum((1, 2)).min())} .. {int(dead.sum((1, 2)).max())} of 16; "
          f"frames that cull something {int(dead.any((1, 2)).sum())}, that keep something {int((~dead).any((1, 2)).sum())}")
    assert dead.any() and (~dead).any()
    if n > 1:
        assert dead.any((1, 2)).sum() > n // 2 and len({d.tobytes() for d in dead}) > 2
    if n == 70:
        assert dead[64:].any() and (~dead[64:]).any()
    check_all_three(backend, sc)


def test_larger_image_after_a_smaller_one_on_the_same_handle(backend):
    """The map buffer belongs to the handle and grows: a sweep of 64 x 64 images, then one of 128 x 128 images on the same
    volume, equal to the frame-by-frame calls in the same order."""
    small, large = many_scene(3, 64), many_scene(3, 128)
    for sc in (small, large):
        dead = np.stack([model(sc, k)[1][0] for k in range(3)])
        assert dead.any() and (~dead).any()
    be = backend
    per, bat = volume(be, small), volume(be, small)
    for sc in (small, large):
        integrate_frames(be, per, sc)
        integrate_batch(be, bat, sc)
    assert per.status()[1] == bat.status()[1] == small.ref.block_updates + large.ref.block_updates
    assert_same_volume(per, bat)
    check_all_three(be, large)
