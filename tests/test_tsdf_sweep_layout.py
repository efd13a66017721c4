"""The lane mapping of the batch sweep (k_tsdf_integrate_batch): a work item is (block, x-quarter), wave w of the workgroup owns
the micro-column (xq, yq = w), lane (lz, lx, ly) keeps the voxels (4 xq + lx, 4 w + ly, 4 j + lz), j = 0 .. 3, and walks the
frames of the block through a two-deep pipeline.  Every case runs on both back-ends and asks for the same thing: the batch
sweep == the frame-by-frame calls == the oracle, bit for bit, on the block set, tsdf, weight, the integer colour sums and
block_updates.  The oracle keeps the colour as an f64 running mean; mean * weight is an integer to ~1e-10, so its sums are
recovered exactly by rounding and compared as integers.

The shapes are the smallest at which the mapping can go wrong; what a case is there for is asserted first on the oracle's
result or on ``probe`` of test_tsdf_edges.py (Open3D's projection in numpy), so that a scene which does not reach its branch
fails instead of passing vacuously.  References are computed once per scene (``scene``), shared between the back-ends and
with the cases of test_tsdf_edges.py that use the same scene, and never modified.
"""
import numpy as np
import pytest

from test_tsdf_edges import (ROTS, Scene, assert_same_volume, batch_scene, colours, extrinsic, inside_scene, integrate_batch,
                             integrate_frames, probe, rotation, scene, touched, volume)

VL = 1.0 / 64                       # voxel length of the one-block scenes: block (0, 0, 0) is [0, 0.25]^3
BLOCK = (0, 0, 0)


def sums_of(ref):
    """the oracle's export with the colour as integer sums: keys, tsdf, weight, sums"""
    rk, rt, rw, rc = ref.export()
    s = rc * rw[..., None]
    assert np.abs(s - np.rint(s)).max(initial=0.0) < 1e-6
    return rk, rt, rw, np.rint(s).astype(np.uint32)


def blocks_of(arrs):
    keys = arrs[0]
    return {tuple(k): tuple(a[i] for a in arrs[1:]) for i, k in enumerate(keys.tolist())}


def check_all_three(be, sc):
    """batch == frame by frame == oracle, bit for bit -> (per-frame volume's blocks, batch volume's blocks, oracle's blocks)"""
    assert sum(sc.counts) == sc.ref.block_updates > 0
    per, bat = volume(be, sc), volume(be, sc)
    integrate_frames(be, per, sc)
    integrate_batch(be, bat, sc)
    assert per.status()[1] == bat.status()[1] == sc.ref.block_updates
    assert_same_volume(per, bat)
    want = blocks_of(sums_of(sc.ref))
    out = []
    for vol in (per, bat):
        got = blocks_of(vol.download())
        assert set(got) == set(want)
        for k, (t, w, c) in got.items():
            rt, rw, rs = want[k]
            assert np.array_equal(w, rw), k
            assert np.array_equal(t.view(np.uint32), rt.view(np.uint32)), k
            if sc.color:
                assert np.array_equal(c, rs), k
        out.append(got)
    return out[0], out[1], want


# ---- 1. one block, every lane position of every wave on a pixel of its own ------------------------------------------------------
def lanes_pose(roll):
    """A camera 4 units from the centre of block (0, 0, 0), looking almost along z: at 20 px per voxel a step in x / y moves the
    pixel by one voxel pitch, a step in z by about a quarter / a sixteenth of it (tilts of 14 and 2.5 degrees), so the 4096
    centres fall on 4096 different pixels; the roll turns all three voxel axes away from the image axes."""
    R = rotation((0, 0, 1), roll) @ rotation((0, 1, 0), 14.0) @ rotation((1, 0, 0), 2.5)
    return extrinsic(R, np.full(3, 8 * VL) - R.T @ np.array([0.0, 0.0, 4.0]))


def lanes_scene(only_quarter=None):
    def make():
        W = H = 560
        f = 20 * 64 * 4.0
        K = (W, H, f, 1.03 * f, W / 2 + 0.3, H / 2 - 0.4)
        rng = np.random.default_rng(41)
        depth = (4.0 + 0.02 * np.sin(np.arange(W) / 37.0)[None, :] + 0.02 * np.cos(np.arange(H) / 23.0)[:, None]).astype(np.float32)
        frames = [(depth.copy(), colours(rng, W, H), lanes_pose(roll)) for roll in (17.0, 11.0, 0.0)]
        masks = None
        if only_quarter is not None:
            # depth only where the voxels of ONE x-quarter of the block look, in every frame
            full = Scene(K, frames, VL, 0.25)
            masks = []
            for k in range(len(frames)):
                p = probe(full, k, [BLOCK])
                m = np.zeros((H, W), np.uint8)
                sel = np.zeros((16, 16, 16), bool)
                sel[4 * only_quarter:4 * only_quarter + 4] = True
                m[p["v"][0][sel], p["u"][0][sel]] = 1
                masks.append(m)
        return Scene(K, frames, VL, 0.25, masks=masks, max_blocks=512)
    return scene(("sweep-lanes", only_quarter), make)


def test_one_block_every_lane_position_has_its_own_pixel(backend):
    """Block (0, 0, 0) fully inside the frustum of a camera no voxel axis is parallel to: every (lz, lx, ly, j) of every wave of
    every x-quarter projects to a pixel of its own and is updated with that pixel's depth and colour, so a lane that took
    another lane's voxel, pixel or chain position cannot give the right block.  Each x-quarter (= work item) on its own."""
    sc = lanes_scene()
    for k in range(len(sc.frames)):
        p = probe(sc, k, [BLOCK])
        assert BLOCK in touched(sc, k) and p["acc"].all() and p["upd"].all()
        if k == 0:
            assert len(np.unique(p["v"] * sc.K[0] + p["u"])) == 4096
            assert len(np.unique(p["sample"])) > 2000
    per, bat, want = check_all_three(backend, sc)
    print(f"lanes: {len(want)} blocks, per frame {sc.counts}")
    for xq in range(4):
        for name, a, b, r in zip(("tsdf", "weight", "colour sums"), per[BLOCK], bat[BLOCK], want[BLOCK]):
            a, b, r = (x.reshape((16, 16, 16) + x.shape[1:])[4 * xq:4 * xq + 4] for x in (a, b, r))
            assert np.array_equal(b.view(np.uint32), r.view(np.uint32)), f"x-quarter {xq}: {name} of the batch sweep against the oracle"
            assert np.array_equal(b.view(np.uint32), a.view(np.uint32)), f"x-quarter {xq}: {name} of the batch sweep against the per-frame path"
        assert np.all(want[BLOCK][1].reshape(16, 16, 16)[4 * xq:4 * xq + 4] == len(sc.frames))


@pytest.mark.parametrize("xq", [0, 2])
def test_only_one_x_quarter_of_the_block_receives_updates(backend, xq):
    """The depth is masked down to the pixels that the voxels of one x-quarter of block (0, 0, 0) look at: the other three work
    items of the block walk the same frames and must leave their voxels alone (x-quarter 0 also counts the block's updates)."""
    sc = lanes_scene(xq)
    for k in range(len(sc.frames)):
        assert BLOCK in touched(sc, k)
        upd = probe(sc, k, [BLOCK])["upd"][0]
        assert upd[4 * xq:4 * xq + 4].all() and upd.sum() == 1024
    _, bat, want = check_all_three(backend, sc)
    w = bat[BLOCK][1].reshape(16, 16, 16)
    assert np.all(w[4 * xq:4 * xq + 4] == len(sc.frames)) and w.sum() == 1024 * len(sc.frames)


# ---- 2. the frame pipeline's exits, and frame-mask bit 63 -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_frames_per_block_1_2_3_and_64(backend, n):
    """A block touched by 1, 2 and 3 frames leaves the two-deep frame pipeline after its head, its first and its second stage;
    with 64 frames in one call bit 63 of the frame mask is used (a block only frame 63 touches), next to blocks many frames touch."""
    sc = batch_scene(n, False)
    sets = [touched(sc, k) for k in range(n)]
    by_count = {}
    for key in set().union(*sets):
        by_count.setdefault(sum(key in s for s in sets), []).append(key)
    print(f"{n} frames: blocks by the number of frames that touch them { {c: len(v) for c, v in sorted(by_count.items())} }")
    if n <= 3:
        assert n in by_count and all(sc.counts)
    else:
        only_63 = sets[63] - set().union(*sets[:63])
        assert only_63 and max(by_count) > 3
    check_all_three(backend, sc)


# ---- 3. a surface across block borders in x and in z ----------------------------------------------------------------------------
def border_scene():
    def make():
        W, H = 37, 23
        rng = np.random.default_rng(43)
        K = (W, H, 31.0, 29.0, 18.3, 11.6)
        corner = np.array([0.5, 0.25, 0.5])              # on the edge shared by blocks (0,0,0), (1,0,0), (0,0,1) and (1,0,1) at voxel 1/32
        frames = []
        for k in range(2):
            R = ROTS[k]
            frames.append((np.full((H, W), 0.8, np.float32), colours(rng, W, H), extrinsic(R, corner - R.T @ np.array([0.0, 0.0, 0.8]))))
        return Scene(K, frames, 1.0 / 32, 0.06, max_blocks=256)
    return scene("sweep-border", make)


def test_surface_across_the_block_border_in_x_and_in_z(backend):
    """Neighbouring blocks in x (other x-quarters, the same micro-column position) and in z (the chain starts again at z = 0 of
    the upper block): voxels on both sides of either face are updated."""
    sc = border_scene()
    _, _, want = check_all_three(backend, sc)
    w = {k: want[k][1].reshape(16, 16, 16) for k in ((0, 0, 0), (1, 0, 0), (0, 0, 1))}
    across_x = (w[(0, 0, 0)][15] > 0) & (w[(1, 0, 0)][0] > 0)
    across_z = (w[(0, 0, 0)][:, :, 15] > 0) & (w[(0, 0, 1)][:, :, 0] > 0)
    print(f"border: {len(want)} blocks, voxel pairs updated across the x face {int(across_x.sum())}, across the z face {int(across_z.sum())}")
    assert across_x.sum() > 10 and across_z.sum() > 10


# ---- 4. the smallest images, with and without colour, with a mask ---------------------------------------------------------------
def small_image_scene(W, H, color, use_mask):
    base = inside_scene(W, H, color)
    if not use_mask:
        return base

    def make():
        rng = np.random.default_rng(47 * W + H)
        masks = []
        for k in range(len(base.frames)):
            m = (rng.uniform(size=(H, W)) > 0.3).astype(np.uint8)
            m[0, 0] = m[-1, -1] = m[0, -1] = 1                   # the corners stay, the last pixel among them
            if W * H == 1 and k == 1:
                m[0, 0] = 0                                      # the only pixel masked out: that frame touches nothing
            masks.append(m)
        return Scene(base.K, base.frames, base.voxel, base.trunc, color=color, masks=masks, max_blocks=base.max_blocks)
    return scene(("sweep-small", W, H, color), make)


@pytest.mark.parametrize("W,H", [(1, 1), (37, 23), (65, 5)])
@pytest.mark.parametrize("color,use_mask", [(True, False), (True, True), (False, True)])
def test_smallest_images_with_and_without_colour_and_mask(backend, W, H, color, use_mask):
    """1 x 1, 37 x 23 and 65 x 5 pixels under three cameras inside the volume: pixels u = 0, u = W - 1 and v = H - 1 are sampled,
    and the last pixel's colour (the bytewise read: no byte follows it) is what some voxel is updated with."""
    sc = small_image_scene(W, H, color, use_mask)
    first = last_col = last_row = last = 0
    for k in range(len(sc.frames)):
        p = probe(sc, k, touched(sc, k)) if sc.counts[k] else None
        if p is None:
            continue
        first += int((p["upd"] & (p["u"] == 0)).sum())
        last_col += int((p["upd"] & (p["u"] == W - 1)).sum())
        last_row += int((p["upd"] & (p["v"] == H - 1)).sum())
        last += int((p["upd"] & (p["u"] == W - 1) & (p["v"] == H - 1)).sum())
    print(f"{W}x{H} colour {color} mask {use_mask}: blocks per frame {sc.counts}, updates through u = 0 / u = W - 1 / v = H - 1 / the last "
          f"pixel: {first} / {last_col} / {last_row} / {last}")
    assert min(first, last_col, last_row, last) > 0
    if use_mask:
        assert any((m == 0).any() for m in sc.masks)
    check_all_three(backend, sc)
