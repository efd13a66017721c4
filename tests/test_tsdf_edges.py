"""The TSDF integrator at its edges, per frame and in batches, on both back-ends and with the parity suite's own criteria
(``compare`` of test_tsdf_parity.py: block set, blocks integrated per frame and weights exact, tsdf bit for bit, integer
colour sums within 1e-9 of the f64 running mean).  The reference is ``oracle.ScalableTSDFVolume`` fed the same frames in
the same order; a case about the batch path is also compared bit for bit with the per-frame path of the same back-end.

What the sphere-and-ring scenes of the parity, batch and mesh suites never reach: a camera inside the volume with voxels
behind it, full-frame depth up to every border and the last pixel, fx != fy with an off-centre non-integer principal
point, every sampling stride on sizes that are not its multiple, the wave de-duplication of the touch pass at every lane
position, batches of 0 .. 130 frames (two chunks and a rest) with blocks only one frame touches, per-frame and batch calls
mixed on one handle, the depth conversion one ulp either side of its thresholds and at non-finite depths, block indices in
the thousands and across -1 | 0, and the overflow flags 2 and 4.

A reference volume is computed once per scene and shared between the back-ends (``Scene.reference``); it is never
modified.  What a case is there for is asserted first, on the oracle's result or on the few lines of Open3D's projection
restated in numpy below (``frame_boxes``: the f64 back-projection of the touch pass, ``probe``: the f32 projection of the
sweep), so a case whose input does not reach its branch fails instead of passing vacuously; the figures are printed
(``-s``; profiles/tsdf_edges.txt).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle
from gs2mesh_amd.integration import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume, TSDFVolumeColorType
from gs2mesh_amd.rasterizer import _ptr
from test_tsdf_parity import compare

F32 = np.float32
INF = float("inf")
_SCENES = {}


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def extrinsic(R, centre):
    """world -> camera of a camera at ``centre`` with orientation R"""
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ np.asarray(centre, np.float64)
    return E


# three general rotations, roll included
ROTS = [rotation((0.3, -0.5, 0.8), 37.0), rotation((-0.7, 0.2, 0.4), 141.0) @ rotation((0, 0, 1), 25.0),
        rotation((0.1, 0.9, -0.3), -73.0)]


class Scene:
    """frames [(depth f32 [H,W], colour u8 [H,W,3], E 4x4)], the intrinsics K = (W, H, fx, fy, cx, cy) and the volume's and the
    conversion's parameters; everything the oracle says about them is computed once and kept"""

    def __init__(self, K, frames, voxel, trunc, stride=4, color=True, depth_scale=1.0, depth_trunc=INF, masks=None,
                 min_depth=0.0, max_blocks=512):
        self.K, self.frames, self.voxel, self.trunc, self.stride, self.color = K, frames, voxel, trunc, stride, color
        self.depth_scale, self.depth_trunc, self.min_depth, self.max_blocks = depth_scale, depth_trunc, min_depth, max_blocks
        self.masks = masks if masks is not None else [None] * len(frames)
        W, H = K[0], K[1]
        for (d, c, E), m in zip(frames, self.masks):
            assert d.shape == (H, W) and d.dtype == np.float32 and c.shape == (H, W, 3) and c.dtype == np.uint8
            assert c.flags["C_CONTIGUOUS"] and c.nbytes == H * W * 3             # no byte behind the last pixel
            assert m is None or (m.shape == (H, W) and m.dtype == np.uint8)
            for a in (d, c, E) + (() if m is None else (m,)):
                a.setflags(write=False)
        self._ref = None

    def converted(self, k, depth=None):
        """the depth of frame k as the integrator sees it: TSDF.run's preprocessing as run_both of test_tsdf_parity.py spells
        it, then the oracle's own RGBD conversion"""
        d = (self.frames[k][0] if depth is None else depth).copy()
        with np.errstate(invalid="ignore"):
            if self.masks[k] is not None:
                d = d * (self.masks[k] != 0)
            if self.min_depth > 0:
                d = np.where(d < np.float32(self.min_depth), 0, d).astype(np.float32)
        return oracle.ScalableTSDFVolume.convert_depth(d, self.depth_scale, self.depth_trunc)

    def oracle_run(self, skip=(), edit=None):
        """a fresh oracle volume over the frames in order (without the frames ``skip``; ``edit(k, depth)`` may replace a
        frame's raw depth) -> (volume, blocks integrated per frame)"""
        W, H, fx, fy, cx, cy = self.K
        ref = oracle.ScalableTSDFVolume(self.voxel, self.trunc, int(self.color), depth_sampling_stride=self.stride)
        counts = []
        for k, (d, c, E) in enumerate(self.frames):
            if k in skip:
                counts.append(0)
                continue
            dd = self.converted(k, None if edit is None else edit(k, d))
            counts.append(ref.integrate(dd, c if self.color else None, W, H, fx, fy, cx, cy, E))
        return ref, counts

    @property
    def reference(self):
        if self._ref is None:
            self._ref = self.oracle_run()
        return self._ref

    @property
    def ref(self):
        return self.reference[0]

    @property
    def counts(self):
        return self.reference[1]

    def keys(self):
        return set(map(tuple, self.ref.export()[0].tolist()))


def scene(key, make):
    if key not in _SCENES:
        _SCENES[key] = make()
    return _SCENES[key]


def colours(rng, W, H):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- the few lines of Open3D's projection, in numpy ---------------------------------------------------------------------------
def frame_boxes(sc, k):
    """PointCloudFactory.cpp CreatePointCloudFromFloatDepthImage + ScalableTSDFVolume::LocateVolumeUnit in f64 for the strided
    pixels of frame k, in the touch pass's order (index = strided row * nx + strided column): valid [n], lo [n,3], hi [n,3]"""
    W, H, fx, fy, cx, cy = sc.K
    ii, jj = np.arange(0, H, sc.stride), np.arange(0, W, sc.stride)
    z = sc.converted(k)[np.ix_(ii, jj)].astype(np.float64)
    valid = z > 0
    z = np.where(valid, z, 1.0)
    x, y = (jj[None, :] - cx) * z / fx, (ii[:, None] - cy) * z / fy
    pose = np.linalg.inv(sc.frames[k][2])
    L = sc.voxel * 16
    lo, hi = [], []
    for r in range(3):
        pw = pose[r, 0] * x + pose[r, 1] * y + pose[r, 2] * z + pose[r, 3] * 1.0
        lo.append(np.floor((pw - sc.trunc) / L).astype(np.int64).reshape(-1))
        hi.append(np.floor((pw + sc.trunc) / L).astype(np.int64).reshape(-1))
    return valid.reshape(-1), np.stack(lo, 1), np.stack(hi, 1)


def touched(sc, k):
    """the set of blocks frame k touches; its size is what the oracle reports as blocks integrated in that frame"""
    valid, lo, hi = frame_boxes(sc, k)
    out = set()
    for i in np.flatnonzero(valid):
        out.update(itertools.product(*(range(lo[i, a], hi[i, a] + 1) for a in range(3))))
    return out


def wave_figures(sc, k):
    """per 64 strided pixels with a valid one among them: (valid lanes, boxes that differ from a valid previous lane's = what
    the touch pass stages, blocks of the union box)"""
    valid, lo, hi = frame_boxes(sc, k)
    out = []
    for w in range(0, len(valid), 64):
        v, l, h = valid[w:w + 64], lo[w:w + 64], hi[w:w + 64]
        if not v.any():
            continue
        same = np.zeros(len(v), bool)
        same[1:] = v[1:] & v[:-1] & np.all(l[1:] == l[:-1], 1) & np.all(h[1:] == h[:-1], 1)
        ext = h[v].max(0) - l[v].min(0) + 1
        out.append((int(v.sum()), int((v & ~same).sum()), tuple(int(e) for e in ext)))
    return out


def probe(sc, k, keys):
    """UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier in numpy f32 for the voxels [x, y, z] of the blocks
    ``keys`` under frame k: camera depth pc2, the pixel coordinates u_f / v_f the accept test sees, the pixel, whether the
    voxel is updated and the tsdf sample it is updated with"""
    W, H, fx, fy, cx, cy = sc.K
    E = sc.frames[k][2].astype(np.float32)
    keys = np.asarray(sorted(keys), np.int64).reshape(-1, 3)
    vl = F32(sc.voxel)
    half = vl * F32(0.5)
    L = sc.voxel * 16
    i16 = np.arange(16, dtype=np.float32)
    lin = half + vl * i16                                                # f32
    org = keys.astype(np.float64) * L
    p0 = (lin[None, :].astype(np.float64) + org[:, 0:1]).astype(np.float32)[:, :, None]        # [n,16,1]
    p1 = (lin[None, :].astype(np.float64) + org[:, 1:2]).astype(np.float32)[:, None, :]        # [n,1,16]
    p2 = (np.float64(half) + org[:, 2]).astype(np.float32)[:, None, None]
    pc = [E[r, 0] * p0 + E[r, 1] * p1 + E[r, 2] * p2 + E[r, 3] * F32(1.0) for r in range(3)]
    step = [E[r, 2] * vl for r in range(3)]
    chain = [[], [], []]
    for z in range(16):
        for r in range(3):
            chain[r].append(pc[r])
            pc[r] = pc[r] + step[r]
    pc0, pc1, pc2 = (np.stack(c, -1) for c in chain)                    # [n,16,16,16]
    front = pc2 > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u_f = pc0 * F32(fx) / pc2 + F32(cx) + F32(0.5)
        v_f = pc1 * F32(fy) / pc2 + F32(cy) + F32(0.5)
    in_u = (u_f >= F32(0.0001)) & (u_f < F32(W - F32(0.0001)))
    in_v = (v_f >= F32(0.0001)) & (v_f < F32(H - F32(0.0001)))
    acc = front & in_u & in_v
    u = np.where(acc, u_f, 0).astype(np.int64)
    v = np.where(acc, v_f, 0).astype(np.int64)
    d = sc.converted(k)[v, u]
    xx, yy = (u.astype(np.float32) - F32(cx)) * (F32(1.0) / F32(fx)), (v.astype(np.float32) - F32(cy)) * (F32(1.0) / F32(fy))
    mult = np.sqrt(xx * xx + yy * yy + F32(1.0))
    with np.errstate(invalid="ignore"):
        sdf = (d - pc2) * mult
        upd = acc & (d > 0) & (sdf > -F32(sc.trunc))
        sample = np.minimum(F32(1.0), sdf * (F32(1.0) / F32(sc.trunc)))
    return dict(front=front, in_u=in_u, in_v=in_v, acc=acc, u_f=u_f, v_f=v_f, u=u, v=v, upd=upd, sample=sample)


# ---- the back-end under test ---------------------------------------------------------------------------------------------------
def volume(be, sc, max_blocks=None):
    ct = TSDFVolumeColorType.RGB8 if sc.color else TSDFVolumeColorType.NoColor
    return ScalableTSDFVolume(sc.voxel, sc.trunc, ct, depth_sampling_stride=sc.stride, max_blocks=max_blocks or sc.max_blocks,
                              lib=be.lib)


def rgbd(be, sc, k):
    d, c, _ = sc.frames[k]
    if sc.depth_scale == 1.0 and sc.depth_trunc == INF:
        return RGBDImage(be.dev(c.copy()), be.dev(d.copy()))            # the constructor's defaults: scale 1, truncation inf
    return RGBDImage(be.dev(c.copy()), be.dev(d.copy()), depth_scale=sc.depth_scale, depth_trunc=sc.depth_trunc)


def intrinsic(sc):
    return PinholeCameraIntrinsic(*sc.K)


def integrate_frames(be, vol, sc, lo=0, hi=None, check_counts=True):
    for k in range(lo, len(sc.frames) if hi is None else hi):
        before = vol.status()[1]
        m = sc.masks[k]
        vol.integrate(rgbd(be, sc, k), intrinsic(sc), sc.frames[k][2], mask=None if m is None else be.dev(m.copy()),
                      min_depth=sc.min_depth)
        if check_counts:
            assert vol.status()[1] - before == sc.counts[k], f"blocks integrated in frame {k}"


def integrate_batch(be, vol, sc, lo=0, hi=None):
    ks = list(range(lo, len(sc.frames) if hi is None else hi))
    masks = None if all(sc.masks[k] is None for k in ks) else [None if sc.masks[k] is None else be.dev(sc.masks[k].copy()) for k in ks]
    vol.integrate_batch([rgbd(be, sc, k) for k in ks], intrinsic(sc), [sc.frames[k][2] for k in ks], masks=masks,
                        min_depth=sc.min_depth)


def assert_same_volume(a, b):
    """two volumes of one back-end hold the same blocks with the same bits"""
    ka, ta, wa, ca = a.download()
    kb, tb, wb, cb = b.download()
    ib = {tuple(k): i for i, k in enumerate(kb.tolist())}
    assert set(ib) == set(map(tuple, ka.tolist()))
    order = np.array([ib[tuple(k)] for k in ka.tolist()], np.int64)
    np.testing.assert_array_equal(wb[order], wa)
    np.testing.assert_array_equal(tb[order].view(np.uint32), ta.view(np.uint32))
    np.testing.assert_array_equal(cb[order], ca)
    assert a.status()[1] == b.status()[1]


def integrate(be, vol, sc, entry, check_counts=True):
    if entry == "frame":
        integrate_frames(be, vol, sc, check_counts=check_counts)
    else:
        integrate_batch(be, vol, sc)


def check(be, sc, batch=True):
    """the per-frame path against the oracle (blocks integrated frame by frame included), the batch path against both"""
    assert sum(sc.counts) == sc.ref.block_updates > 0
    per = volume(be, sc)
    integrate_frames(be, per, sc)
    n = compare(per, sc.ref, color=sc.color)
    assert per.status()[1] == sc.ref.block_updates
    if batch:
        bat = volume(be, sc)
        integrate_batch(be, bat, sc)
        assert bat.status()[1] == sc.ref.block_updates
        assert_same_volume(per, bat)
        compare(bat, sc.ref, color=sc.color)
    return n


# ---- 1. camera inside the volume, full-frame depth -----------------------------------------------------------------------------
def inside_scene(W, H, color):
    def make():
        rng = np.random.default_rng(100 * W + H)
        K = (W, H, 0.8 * W + 1.5, 1.1 * H + 0.7, 0.31 * W, 0.68 * H)     # fx != fy, principal point non-integer and off-centre
        n = W * H
        ramp = np.linspace(0.03, 1.2, n).astype(np.float32) if n > 1 else None
        frames = []
        for k, R in enumerate(ROTS):
            if n == 1:
                d = np.full((1, 1), (0.03, 0.45, 1.2)[k], np.float32)
            else:
                d = (ramp.reshape(H, W), ramp[::-1].reshape(H, W), ramp.reshape(W, H).T)[k]
            frames.append((np.ascontiguousarray(d), colours(rng, W, H), extrinsic(R, (0.11 - 0.05 * k, -0.07, 0.05 + 0.03 * k))))
        return Scene(K, frames, 1.0 / 32, 0.06, color=color, max_blocks=768)
    return scene(("inside", W, H, color), make)


@pytest.mark.parametrize("W,H,color", [(1, 1, True), (37, 23, True), (65, 5, True), (37, 23, False)])
def test_camera_inside_the_volume_full_frame_depth(backend, W, H, color):
    """Every pixel valid up to row 0, column 0, the last row, the last column and the last pixel; three cameras with roll
    inside the blocks they touch; fx != fy; the colour buffer ends with the last pixel (the bytewise read)."""
    sc = inside_scene(W, H, color)
    fig = dict(behind=0, last=0, clamped=0, below=0, left=[0, 0], right=[0, 0], top=[0, 0], bottom=[0, 0])
    for k in range(len(sc.frames)):
        assert np.all(sc.converted(k) > 0)                                # full-frame depth, the borders included
        keys = touched(sc, k)
        assert len(keys) == sc.counts[k]
        p = probe(sc, k, keys)
        fig["behind"] += int((~p["front"]).sum())                          # pc2 <= 0 in a touched block
        fig["last"] += int((p["upd"] & (p["u"] == W - 1) & (p["v"] == H - 1)).sum())      # the last pixel, gathered with colour
        fig["clamped"] += int((p["upd"] & (p["sample"] == 1)).sum())
        fig["below"] += int((p["upd"] & (p["sample"] < 1)).sum())
        fu, fv = p["front"] & p["in_v"], p["front"] & p["in_u"]         # the other coordinate passes: THIS border decides
        for name, ok, c, size in (("left", fu, p["u_f"], None), ("right", fu, p["u_f"], W), ("top", fv, p["v_f"], None),
                                  ("bottom", fv, p["v_f"], H)):
            if size is None:
                fig[name][0] += int((ok & (c >= -0.5) & (c < F32(0.0001))).sum())        # refused
                fig[name][1] += int((ok & (c >= F32(0.0001)) & (c < 0.5)).sum())         # accepted
            else:
                fig[name][0] += int((ok & (c >= F32(size - F32(0.0001))) & (c < size + 0.5)).sum())
                fig[name][1] += int((ok & (c < F32(size - F32(0.0001))) & (c >= size - 0.5)).sum())
    print(f"inside {W}x{H} colour={color}: blocks {sc.ref.num_blocks}, per frame {sc.counts}, behind-camera voxels {fig['behind']}, "
          f"updates through the last pixel {fig['last']}, samples clamped to 1 / below 1 {fig['clamped']} / {fig['below']}, "
          f"border voxels refused / accepted: left {fig['left']} right {fig['right']} top {fig['top']} bottom {fig['bottom']}")
    assert fig["behind"] > 0 and fig["last"] > 0 and fig["clamped"] > 0 and fig["below"] > 0
    for name in ("left", "right", "top", "bottom"):
        assert min(fig[name]) > 0, name
    check(backend, sc)


# ---- 2. the sampling stride ---------------------------------------------------------------------------------------------------
def stride_scene(stride, W, H):
    def make():
        rng = np.random.default_rng(1000 * stride + 10 * W + H)
        K = (W, H, 0.35 * W + 2.0, 0.5 * H + 2.5, 0.45 * W + 0.3, 0.55 * H - 0.2)
        frames = []
        for k in range(2):
            d = rng.uniform(0.5, 1.1, (H, W)).astype(np.float32)
            frames.append((d, colours(rng, W, H), extrinsic(ROTS[k], (0.2, 0.1 * k, -0.1))))
        return Scene(K, frames, 1.0 / 64, 0.04, stride=stride, max_blocks=1024)
    return scene(("stride", stride, W, H), make)


@pytest.mark.parametrize("stride,W,H", [(1, 7, 5), (2, 12, 8), (2, 13, 7), (3, 15, 9), (3, 16, 11), (4, 16, 12), (4, 18, 13),
                                        (5, 20, 10), (5, 22, 14), (7, 21, 14), (7, 23, 16), (40, 37, 23)])
def test_every_sampling_stride(backend, stride, W, H):
    """Strides 1 .. 7 on sizes that are and are not their multiple (the strided grid is rounded UP), and a stride larger
    than the image: only pixel (0, 0) is sampled."""
    sc = stride_scene(stride, W, H)
    nx, ny = -(-W // stride), -(-H // stride)
    for k in range(len(sc.frames)):
        valid, _, _ = frame_boxes(sc, k)
        assert valid.all() and len(valid) == nx * ny and len(touched(sc, k)) == sc.counts[k]
    if stride > max(W, H):
        assert nx == ny == 1
    print(f"stride {stride} on {W}x{H}: grid {nx}x{ny}, blocks per frame {sc.counts}")
    check(backend, sc)


def last_strided_scene():
    def make():
        W, H = 37, 23
        rng = np.random.default_rng(7)
        K = (W, H, 30.0, 26.0, 17.2, 12.4)
        E = extrinsic(ROTS[0], (0.1, 0.0, -0.2))
        frames = []
        for (i, j) in ((8, 36), (20, 12), (8, 35), (21, 12)):    # last strided column, last strided row, two pixels off the grid
            d = np.zeros((H, W), np.float32)
            d[i, j] = 0.8
            frames.append((d, colours(rng, W, H), E))
        return Scene(K, frames, 1.0 / 64, 0.04, max_blocks=64)
    return scene("last-strided", make)


def test_last_strided_column_and_row_and_pixels_off_the_grid(backend):
    """W = 37, H = 23, stride 4: the strided grid is 10 x 6, its last column is image column 36 and its last row is image row
    20.  One valid pixel there is the frame's whole block set; one valid pixel next to it, off the grid, touches nothing --
    and the blocks its depth lies in (allocated by the frames before) are then not swept."""
    sc = last_strided_scene()
    assert -(-37 // 4) == 10 and 36 == 9 * 4 and -(-23 // 4) == 6 and 20 == 5 * 4
    for k, (i, j) in enumerate(((8, 36), (20, 12))):
        def without(kk, d, k=k, i=i, j=j):
            if kk != k:
                return d
            e = d.copy()
            e[i, j] = 0
            return e
        assert sc.counts[k] > 0 and sc.oracle_run(edit=without)[1][k] == 0       # deleting the pixel empties the frame's block set
    assert sc.counts[2] == sc.counts[3] == 0
    every_pixel = Scene(sc.K, [sc.frames[2]], sc.voxel, sc.trunc, stride=1)       # what (8, 35) would touch were it sampled
    assert touched(every_pixel, 0) & touched(sc, 0)   # blocks that frame 0 allocated: there, and not swept by frame 2
    print(f"last strided column / row: blocks per frame {sc.counts}")
    check(backend, sc)
    alone = volume(backend, sc)                       # an off-grid pixel on a fresh handle: nothing at all
    integrate_frames(backend, alone, sc, 2, 4)
    assert alone.status() == (0, 0, 0)
    integrate_batch(backend, alone, sc, 2, 4)
    assert alone.status() == (0, 0, 0)


# ---- 3. wave de-duplication in the touch pass ----------------------------------------------------------------------------------
def row_scene(name):
    """one image row of 130 pixels at stride 1: three waves of the touch pass, the last one of 2 lanes"""
    def make():
        W, H = 130, 1
        rng = np.random.default_rng(11)
        d = np.zeros((H, W), np.float32)
        fx, R = 4000.0, ROTS[0]
        if name.startswith("single"):
            d[0, int(name[6:])] = 0.7
        elif name == "one-box":
            d[0, 64:128] = 0.7
        elif name == "checkerboard":
            fx = 40.0
            d[0, 1::2] = np.linspace(0.4, 1.3, 65).astype(np.float32)
        elif name == "pair-then-other":
            d[0, 5:7] = 0.7
            d[0, 7] = 1.9
        elif name == "long-union":
            d[0, 70], d[0, 101] = 0.5, 16.0
            R = rotation((1, 0, 0), 28.0) @ rotation((0, 1, 0), -52.0)
        return Scene((W, H, fx, 35.0, 64.3, 0.4), [(d, colours(rng, W, H), extrinsic(R, (0.13, 0.06, 0.02)))], 1.0 / 64, 0.11,
                     stride=1, max_blocks=256)
    return scene(("row", name), make)


@pytest.mark.parametrize("name", ["single0", "single63", "single64", "single127", "single129", "one-box", "checkerboard",
                                  "pair-then-other", "long-union"])
def test_wave_deduplication_of_the_touch_pass(backend, name):
    """Lanes compare their block box with the previous lane's, the distinct ones are staged and every candidate block of the
    wave's union box is tested against them: a single valid lane at each end of each wave (lane 0 has no predecessor), 64
    lanes with one box, valid lanes that all follow an invalid one, an equal pair followed by another box, and two distant
    boxes whose union has three different extents."""
    sc = row_scene(name)
    assert len(touched(sc, 0)) == sc.counts[0] > 0
    figs = wave_figures(sc, 0)
    for n_valid, n_boxes, ext in figs:
        print(f"row {name}: valid lanes {n_valid}, distinct boxes {n_boxes}, union {ext[0]}x{ext[1]}x{ext[2]} = {ext[0] * ext[1] * ext[2]} "
              f"candidates (blocks of the frame: {sc.counts[0]})")
    if name == "checkerboard":                        # all three waves; lane 0 of each is invalid, the last wave has 2 lanes
        assert [f[:2] for f in figs] == [(32, 32), (32, 32), (1, 1)] and not (sc.frames[0][0][0, ::2] > 0).any()
        assert len({tuple(b) for b in np.hstack(frame_boxes(sc, 0)[1:])[1::2].tolist()}) > 8
        check(backend, sc)
        return
    (n_valid, n_boxes, ext), = figs                   # exactly one wave has valid lanes
    if name.startswith("single"):
        assert (n_valid, n_boxes) == (1, 1) and int(name[6:]) in (0, 63, 64, 127, 129)
    elif name == "one-box":
        assert (n_valid, n_boxes) == (64, 1)
    elif name == "pair-then-other":
        assert (n_valid, n_boxes) == (3, 2)
    else:
        assert (n_valid, n_boxes) == (2, 2) and len(set(ext)) == 3 and 5e4 < ext[0] * ext[1] * ext[2] < 2e5
    check(backend, sc)


# ---- 4. batch sizes and the frame mask -------------------------------------------------------------------------------------------
BATCH_ONLY = {63: (5.0, 0.0, 0.0), 64: (0.0, -5.0, 0.0)}       # frames whose camera sits where no other frame looks


def batch_scene(n, use_mask):
    def make():
        W, H = 9, 7
        rng = np.random.default_rng(13)
        K = (W, H, 9.5, 8.0, 3.7, 4.2)
        empty = {0, n // 2, n - 1} - set(BATCH_ONLY) if n >= 5 else set()
        poses = [extrinsic(rotation((0.2, 1.0, 0.1), 4.0 * p) @ ROTS[0], (0.05 * p, 0.02, -0.03 * p)) for p in range(5)]
        frames, masks = [], []
        for k in range(n):
            d = np.zeros((H, W), np.float32) if k in empty else (0.55 + 0.01 * (k % 7) + rng.uniform(0, 0.05, (H, W))).astype(np.float32)
            E = poses[k % 5]                                   # poses repeat: voxels collect one update per repetition
            if k in BATCH_ONLY:
                E = extrinsic(ROTS[1], BATCH_ONLY[k])
            frames.append((d, colours(rng, W, H), E))
            masks.append((rng.uniform(size=(H, W)) > 0.25).astype(np.uint8) if use_mask and k % 3 == 1 else None)
        sc = Scene(K, frames, 1.0 / 32, 0.06, masks=masks, max_blocks=256)
        sc.empty = empty
        return sc
    return scene(("batch", n, use_mask), make)


@pytest.mark.parametrize("n,use_mask", [(0, False), (1, False), (2, True), (63, False), (64, True), (65, False), (130, True)])
def test_batch_sizes_and_the_frame_mask(backend, n, use_mask):
    """Batches of 0 .. 130 frames in one call (above 64 the call splits into chunks of 64: one bit per frame in a block's
    frame mask), frames without a valid pixel first, in the middle and last, a block that only frame 63 touches and one that
    only frame 64 = the first frame of the second chunk touches, masks given for some frames: equal to the per-frame path
    bit for bit and to the oracle."""
    be = backend
    sc = batch_scene(n, use_mask)
    if n == 0:
        vol = volume(be, sc)
        vol.integrate_batch([], intrinsic(sc), [])
        assert vol.status() == (0, 0, 0)
        rc = be.lib.gs2m_tsdf_integrate_batch(vol._h, 0, None, None, None, 9, 7, 9.5, 8.0, 3.7, 4.2, None, 1.0, 1e9, 0.0, None)
        assert rc == 0 and vol.status() == (0, 0, 0)
        return
    for k in sc.empty:
        assert sc.counts[k] == 0
    assert all(c > 0 for k, c in enumerate(sc.counts) if k not in sc.empty)
    all_keys = sc.keys()
    for k in BATCH_ONLY:
        if k < n:
            only = all_keys - set(map(tuple, sc.oracle_run(skip={k})[0].export()[0].tolist()))
            assert len(only) > 0, f"no block that only frame {k} touches"
            print(f"batch of {n}: {len(only)} blocks only frame {k} touches")
    wmax = float(sc.ref.export()[2].max())
    print(f"batch of {n}, masks {use_mask}: blocks {len(all_keys)}, largest weight {wmax:.0f}, empty frames {sorted(sc.empty)}")
    if n == 130:
        assert wmax > 64
    if use_mask:
        assert any(m is None for m in sc.masks) and any(m is not None and (m == 0).any() for m in sc.masks)
    check(be, sc)


# ---- 5. mixed use of one handle ----------------------------------------------------------------------------------------------------
def test_per_frame_and_batch_calls_mixed_on_one_handle(backend):
    """per-frame, batch of 3, per-frame, per-frame, batch of 2, per-frame on one handle (the frame stamps of the per-frame
    path and the frame masks of the batch path side by side) = the oracle fed the nine frames in order; then reset() and
    another scene = a fresh handle."""
    be = backend
    sc = inside_scene(37, 23, True)
    nine = scene("nine", lambda: Scene(sc.K, [sc.frames[k % 3][:2] + (extrinsic(ROTS[k % 3], (0.1 * (k // 3), -0.07, 0.05 * k)),)
                                               for k in range(9)], sc.voxel, sc.trunc, max_blocks=1024))
    assert len(set(nine.counts)) > 1 and nine.ref.export()[2].max() >= 3
    vol = volume(be, nine)
    at = 0
    for how, cnt in (("frame", 1), ("batch", 3), ("frame", 1), ("frame", 1), ("batch", 2), ("frame", 1)):
        (integrate_frames if how == "frame" else integrate_batch)(be, vol, nine, at, at + cnt)
        at += cnt
        assert vol.status()[1] == sum(nine.counts[:at])
    assert at == 9
    compare(vol, nine.ref)
    other = batch_scene(64, True)                    # another scene (other intrinsics, masks) of the handle's stride
    assert other.keys() != nine.keys()
    vol.reset()
    assert vol.status() == (0, 0, 0)
    integrate_frames(be, vol, other, 0, 30)
    integrate_batch(be, vol, other, 30, 64)
    fresh = volume(be, other, max_blocks=nine.max_blocks)
    integrate_batch(be, fresh, other)
    assert_same_volume(vol, fresh)
    compare(vol, other.ref)


# ---- 6. the depth conversion at its thresholds ---------------------------------------------------------------------------------------
BAD = (np.nan, np.inf, -np.inf, -0.5, 0.0)


def nonfinite_scene(use_mask):
    def make():
        W, H = 21, 13
        rng = np.random.default_rng(17)
        K = (W, H, 19.0, 16.5, 8.3, 7.9)
        frames, masks, kinds = [], [], []
        for k in range(2):
            d = np.linspace(0.3, 0.9, W * H).astype(np.float32).reshape(H, W).copy()
            kind = np.full((H, W), -1)
            where = rng.choice(W * H, 70, replace=False)
            kind.reshape(-1)[where] = np.arange(70) % 5
            for n, (i, j) in enumerate(((0, 0), (4, 8), (8, 12), (12, 20), (8, 4))):     # one of each kind on the strided grid
                kind[i, j] = n
            for n, b in enumerate(BAD):
                d[kind == n] = b
            m = None
            if use_mask:
                m = (rng.uniform(size=(H, W)) > 0.3).astype(np.uint8)
                m[0, 0], m[4, 8] = 0, 1                       # NaN * 0 and NaN * 1
            frames.append((d, colours(rng, W, H), extrinsic(ROTS[k], (0.05, 0.02 * k, 0.1))))
            masks.append(m)
            kinds.append(kind)
        sc = Scene(K, frames, 1.0 / 32, 0.06, masks=masks, max_blocks=512)
        sc.kinds = kinds
        return sc
    return scene(("nonfinite", use_mask), make)


@pytest.mark.parametrize("use_mask", [False, True])
def test_nonfinite_negative_and_zero_depths(backend, use_mask):
    """NaN, +inf, -inf, negative and zero depths through a valid frame, without and with a mask (NaN * 0 is NaN), under the
    RGBDImage constructor's own depth_trunc = inf (+inf >= inf: truncated): those pixels touch nothing and update nothing."""
    sc = nonfinite_scene(use_mask)
    assert sc.depth_trunc == INF and sc.depth_scale == 1.0
    on_grid, sampled = np.zeros(5, int), np.zeros(5, int)
    for k in range(2):
        conv, kind = sc.converted(k), sc.kinds[k]
        with np.errstate(invalid="ignore"):
            assert not (conv[kind >= 0] > 0).any() and np.isnan(conv[kind == 0]).all()
            masked = np.zeros_like(kind, bool) if sc.masks[k] is None else sc.masks[k] == 0
            assert np.all(conv[(kind == 1) & ~masked] == 0) and np.isnan(conv[(kind == 1) & masked]).all()       # inf * 0 is NaN too
        if use_mask:
            assert np.isnan(conv[0, 0]) and masked[0, 0] and (conv[masked & (kind < 0)] == 0).all() and (masked & (kind == 1)).any()
        p = probe(sc, k, touched(sc, k))
        for n in range(5):
            on_grid[n] += int((kind[::4, ::4] == n).sum())
            sampled[n] += int((p["acc"] & (kind[p["v"], p["u"]] == n)).sum())
            assert not (p["upd"] & (kind[p["v"], p["u"]] == n)).any()
    print(f"non-finite depths, mask {use_mask}: pixels on the strided grid / voxels that sample them, per kind (nan, +inf, -inf, "
          f"negative, zero): {on_grid.tolist()} / {sampled.tolist()}")
    assert on_grid.min() > 0 and sampled.min() > 0
    # to the reference they are zero depth: the same volume bit for bit
    zeroed = sc.oracle_run(edit=lambda k, d: np.where(sc.kinds[k] >= 0, 0, d).astype(np.float32))[0].export()
    for a, b in zip(zeroed, sc.ref.export()):
        assert np.array_equal(a, b)
    check(backend, sc)


def ulps(x):
    x = F32(x)
    return np.nextafter(x, F32(-INF)), x, np.nextafter(x, F32(INF))


def threshold_scene(kind):
    """a wall at depth ~0.1 whose pixels cycle through three neighbouring floats around a threshold of the conversion"""
    def make():
        W, H = 13, 9
        rng = np.random.default_rng(19)
        K = (W, H, 11.0, 9.5, 5.6, 4.7)
        kw = dict(depth_trunc=INF)
        if kind == "trunc":                                   # depth_trunc = 0.1 is no float: float32(0.1) > 0.1 > the float below
            values, kw = ulps(0.1), dict(depth_trunc=0.1)
        elif kind == "trunc-scaled":                          # raw depths whose f32 quotient by 0.3 lands one ulp below, on and above
            three, values = F32(0.3), []
            cand = [F32(0.1) * three]
            for _ in range(24):
                cand = [np.nextafter(cand[0], F32(-INF))] + cand + [np.nextafter(cand[-1], F32(INF))]
            for target in ulps(0.1):
                hit = [c for c in cand if c / three == target]
                assert hit, "no raw depth whose quotient lands on the threshold"
                values.append(hit[0])
            kw = dict(depth_trunc=0.1, depth_scale=0.3)
        elif kind == "min-at":                                # min_depth equal to a depth value: kept (the comparison is strict)
            values, kw = ulps(0.1), dict(depth_trunc=INF, min_depth=float(F32(0.1)))
        else:                                                 # min_depth one ulp above it: dropped
            values, kw = ulps(0.1), dict(depth_trunc=INF, min_depth=float(ulps(0.1)[2]))
        which = (np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 3
        d = np.asarray(values, np.float32)[which]
        frames = [(d, colours(rng, W, H), extrinsic(ROTS[k], (0.03, 0.01, 0.02 * k))) for k in range(2)]
        sc = Scene(K, frames, 1.0 / 64, 0.04, max_blocks=256, **kw)
        sc.which, sc.values = which, values
        return sc
    return scene(("threshold", kind), make)


@pytest.mark.parametrize("kind,kept", [("trunc", (True, False, False)), ("trunc-scaled", (True, False, False)),
                                       ("min-at", (False, True, True)), ("min-above", (False, False, True))])
def test_depth_conversion_one_ulp_either_side_of_its_thresholds(backend, kind, kept):
    """depth_trunc = 0.1 (a double between two floats) against depths one ulp below, at and above float32(0.1), directly and
    as the quotient by depth_scale = 0.3; min_depth equal to a depth (kept: depth < min is strict) and one ulp above it."""
    sc = threshold_scene(kind)
    conv = sc.converted(0)
    got = tuple(bool((conv[sc.which == n] > 0).all()) for n in range(3))
    none = tuple(bool((conv[sc.which == n] == 0).all()) for n in range(3))
    print(f"threshold {kind}: raw depths {[float(v) for v in sc.values]} -> kept {got}")
    assert got == kept and none == tuple(not x for x in kept)
    if kind.startswith("trunc"):
        assert float(F32(0.1)) > 0.1 > float(ulps(0.1)[0])
    assert all((sc.which[::4, ::4] == n).any() for n in range(3))           # each value is seen by the touch pass
    p = probe(sc, 0, touched(sc, 0))
    assert all((p["acc"] & (sc.which[p["v"], p["u"]] == n)).any() for n in range(3))      # and by the sweep
    check(backend, sc)


# ---- 7. far from the origin, negative block indices ---------------------------------------------------------------------------------
def place_scene(centre):
    def make():
        W, H = 21, 13
        rng = np.random.default_rng(23)
        K = (W, H, 18.0, 15.0, 9.4, 7.2)
        ramp = np.linspace(0.2, 1.0, W * H).astype(np.float32)
        frames = [((ramp if k == 0 else ramp[::-1]).reshape(H, W).copy(), colours(rng, W, H), extrinsic(ROTS[k + 1], centre))
                  for k in range(2)]
        return Scene(K, frames, 0.02, 0.05, max_blocks=512)       # a voxel length that is no binary fraction
    return scene(("place", centre), make)


@pytest.mark.parametrize("centre", [(1000.3, -777.7, 512.1), (0.02, -0.03, 0.01)])
def test_block_indices_in_the_thousands_and_across_zero(backend, centre):
    """A camera a thousand units out (block indices in the thousands: the f64 -> f32 casts of the voxel centres round) and
    one at the origin whose blocks straddle index -1 | 0 on all three axes."""
    sc = place_scene(centre)
    keys = np.array(sorted(sc.keys()))
    print(f"camera at {centre}: block indices {keys.min(0).tolist()} .. {keys.max(0).tolist()}")
    if abs(centre[0]) > 100:
        assert np.all(np.abs(keys).min(0) > 1000) and (keys[:, 1] < 0).all()
        centres = keys[:, None, :] * (16 * sc.voxel) + (np.arange(16)[None, :, None] + 0.5) * sc.voxel
        err = np.abs(centres.astype(np.float32).astype(np.float64) - centres).max() / sc.voxel
        print(f"largest rounding of a voxel centre in f32: {err:.2e} voxels")
        assert err > 1e-4
    else:
        assert np.all(keys.min(0) <= -1) and np.all(keys.max(0) >= 0)
    check(backend, sc)


# ---- 8. the overflow flags nobody raises ---------------------------------------------------------------------------------------------
def small_scene(like):
    """two ordinary frames of at most 8 blocks for a handle made for the scene ``like`` (its voxel, truncation and stride)"""
    def make():
        W, H = 2 * like.stride + 1, like.stride + 2
        rng = np.random.default_rng(37)
        frames = [(rng.uniform(0.78, 0.8, (H, W)).astype(np.float32), colours(rng, W, H), extrinsic(ROTS[k], (0.05, 0.02, 0.01)))
                  for k in range(2)]
        return Scene((W, H, 150.0, 140.0, 0.4 * W, 0.6 * H), frames, like.voxel, like.trunc, stride=like.stride, max_blocks=8)
    return scene(("small", like.voxel, like.trunc, like.stride), make)


def flag4_scene(kind):
    def make():
        rng = np.random.default_rng(29)
        if kind == "far":                                     # unit length 0.5: block index 2^20 is coordinate 524288
            W, H, stride = 1, 1, 4
            d = np.full((1, 1), 600000.0, np.float32)
            K, E = (1, 1, 1.7, 1.3, 0.3, 0.6), extrinsic(np.eye(3), (0, 0, 0))
        else:                                                 # two lanes of one wave, 300 units apart along a diagonal ray
            W, H, stride = 8, 1, 1
            d = np.zeros((1, 8), np.float32)
            d[0, 2], d[0, 5] = 0.5, 300.0
            K, E = (8, 1, 500.0, 500.0, 3.6, 0.4), extrinsic(rotation((1, 0, 0), 35.0) @ rotation((0, 1, 0), -45.0), (0.1, 0, 0))
        return Scene(K, [(d, colours(rng, W, H), E)], 1.0 / 32, 0.06, stride=stride, max_blocks=64)
    return scene(("flag4", kind), make)


@pytest.mark.parametrize("entry", ["frame", "batch"])
@pytest.mark.parametrize("kind", ["far", "union"])
def test_block_index_out_of_range_raises_flag_4(backend, kind, entry):
    """A point beyond block index 2^20, and a wave whose union box holds more than 2^24 blocks: flag 4, by name, no blocks;
    after reset() the handle integrates as a fresh one."""
    be = backend
    sc = flag4_scene(kind)
    valid, lo, hi = frame_boxes(sc, 0)
    ext = hi[valid].max(0) - lo[valid].min(0) + 1
    print(f"flag 4 {kind}: box {lo[valid].min(0).tolist()} .. {hi[valid].max(0).tolist()}, union {int(np.prod(ext))} blocks")
    if kind == "far":
        assert valid.sum() == 1 and hi[valid].max() >= 1 << 20 and np.abs(hi[valid]).max() < 1 << 30
    else:
        assert valid.sum() == 2 and np.prod(ext) > 1 << 24 and np.abs(np.hstack([lo[valid], hi[valid]])).max() < 1 << 20
    vol = volume(be, sc)
    integrate(be, vol, sc, entry, check_counts=False)       # the oracle knows no flags: nothing to count against
    with pytest.raises(RuntimeError, match="out of the"):
        vol.status()
    nb, _, flags = vol.status(raise_on_overflow=False)
    assert flags & 4 and not flags & 3 and nb == 0
    vol.reset()
    assert vol.status() == (0, 0, 0)
    good = small_scene(sc)
    integrate(be, vol, good, entry)
    compare(vol, good.ref)


def crowd_scene():
    def make():
        W, H = 65, 23
        rng = np.random.default_rng(31)
        d = rng.uniform(4.9, 5.1, (H, W)).astype(np.float32)
        return Scene((W, H, 10.0, 10.0, 31.7, 11.2), [(d, colours(rng, W, H), extrinsic(ROTS[2], (0.3, 0.2, 0.1)))], 1.0 / 64, 0.04,
                     stride=1, max_blocks=8)
    return scene("crowd", make)


@pytest.mark.parametrize("entry", ["frame", "batch"])
def test_hash_table_full_raises_flags_1_and_2(backend, entry):
    """max_blocks = 8 gives the smallest table, 1024 cells; a frame that touches more distinct blocks than that fills it: flags
    1 (pool) and 2 (table), the call returns, and after reset() the handle works."""
    be = backend
    sc = crowd_scene()
    n = len(touched(sc, 0))
    print(f"hash table full: the frame touches {n} distinct blocks, the table holds 1024")
    assert n > 1024 and sc.max_blocks == 8
    vol = volume(be, sc)
    integrate(be, vol, sc, entry, check_counts=False)       # the oracle knows no flags: nothing to count against
    with pytest.raises(RuntimeError, match="block pool exhausted.*hash table full"):
        vol.status()
    nb, _, flags = vol.status(raise_on_overflow=False)
    assert flags & 3 == 3 and not flags & 4 and nb == 8
    vol.reset()
    assert vol.status() == (0, 0, 0)
    good = small_scene(sc)
    assert 0 < good.ref.num_blocks <= 8
    integrate(be, vol, good, entry)
    compare(vol, good.ref)


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------------------
def test_singular_extrinsic_and_oversized_batch_images_are_refused(backend):
    """A singular extrinsic is an error of both entry points, not a crash; the batch entry point packs pixel coordinates in 16
    bits and refuses a width or height above 65535 (only the size is passed: no such image exists).  The handle stays usable."""
    be = backend
    sc = last_strided_scene()
    vol = volume(be, sc)
    E = np.eye(4)
    E[2] = 0.0
    assert np.linalg.det(E) == 0
    with pytest.raises(RuntimeError, match="singular extrinsic"):
        vol.integrate(rgbd(be, sc, 0), intrinsic(sc), E)
    with pytest.raises(RuntimeError, match="singular extrinsic"):
        vol.integrate_batch([rgbd(be, sc, 0), rgbd(be, sc, 1)], intrinsic(sc), [sc.frames[0][2], E])
    d, c = be.dev(sc.frames[0][0].copy()), be.dev(sc.frames[0][1].copy())
    dp, cp = (C.c_void_p * 1)(_ptr(d)), (C.c_void_p * 1)(_ptr(c))
    Ep = np.ascontiguousarray(sc.frames[0][2]).ctypes.data_as(C.POINTER(C.c_double))
    for W, H in ((65536, 23), (37, 65536)):
        rc = be.lib.gs2m_tsdf_integrate_batch(vol._h, 1, dp, cp, None, W, H, 30.0, 26.0, 17.2, 12.4, Ep, 1.0, 1e9, 0.0, None)
        assert rc != 0 and b"65535" in be.lib.gs2m_last_error()
    assert vol.status() == (0, 0, 0)
    integrate_frames(be, vol, sc, 0, 2)
    integrate_batch(be, vol, sc, 2, 4)
    compare(vol, sc.ref)
