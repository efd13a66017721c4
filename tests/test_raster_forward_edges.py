"""The forward rasteriser at its thresholds and on non-finite splats, on both back-ends.

Every scene is hand-built for one branch of the code: project_view (near cull, frustum clamp, det == 0, ceil(3 sqrt(lambda)), the
truncating casts of getRect, the zero-area test), the exact tile cull (thr < 0, the box, the collapse), the staging step of the
compositing kernel (box, degenerate, singular, capped) and the reference's three decisions (power > 0, alpha < 1/255,
T' < 1e-4), and quantize_u8.  The camera has an identity pose and exact matrices (power-of-two focal length, depth 2: the centre
of pixel (u, v) projects to (u, v) without rounding), covariances and colours are passed precomputed, so the projected numbers
can be written down; each case first asserts on the ORACLE'S record that it sits where it claims.

Reference: oracle.preprocess / bin_instances / rasterize_forward under the bars of test_raster_parity -- record, radii, rects and
instance lists exact, the image under assert_image_close and assert_image_attributed.  Side points lie 1e-4 relative from a
threshold (ten times the flip window of oracle/parity.py): there the oracle reports no flip pixel and every blend variant, loop
form, tile height and cull level takes the oracle's decision.  At a threshold value itself only the attributed bound applies to
the log2-domain kernel; variant 0 evaluates alpha = o exp(0) and T (1 - alpha) literally and must take the reference's decision.

Non-finite and overflowing splats: the contract of DESIGN.md "Parity" (a) - (e).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer, make_camera
from gs2mesh_amd.sh_utils import RGB2SH
from oracle.parity import CLEAN_BAR
from test_raster_parity import assert_image_attributed, assert_image_close

F32 = np.float32
BG = np.array([0.1, 0.2, 0.3], F32)
THR = F32(1.0) / F32(255.0)          # the reference's 1.0f / 255.0f
REL = 1e-4                           # distance of the side points from a threshold
# (variant, mode, rows): every compositing kernel the library has
BLENDS = [(0, 2, 1), (4, 0, 1), (4, 2, 1), (4, 3, 1), (4, 0, 2), (4, 2, 2), (4, 3, 2)]
CULLS = (0, 1, 2)


def nxt(x, n=1):
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf) if n > 0 else F32(-np.inf))
    return x


# ---- camera and scenes ---------------------------------------------------------------------------------------------------
class Cam:
    """Identity pose, exact matrices: view = I, clip x = (2 f / W) x, y = (2 f / H) y, w = z.  tan(fov) = W / (2 f) exactly."""

    def __init__(self, W, H, f):
        self.image_width, self.image_height, self.f = W, H, float(f)
        self.tanfovx, self.tanfovy = W / (2.0 * f), H / (2.0 * f)
        zn, zf = 0.01, 100.0
        M = np.zeros((4, 4), np.float64)
        M[0, 0], M[1, 1] = 2.0 * f / W, 2.0 * f / H
        M[2, 2], M[2, 3], M[3, 2] = zf / (zf - zn), -(zf * zn) / (zf - zn), 1.0
        self.world_view_transform = np.eye(4, dtype=F32)
        self.full_proj_transform = np.ascontiguousarray(M.T, F32)      # m[4 c + r] = M[r][c]
        self.camera_center = np.zeros(3, F32)

    def place(self, u, v, z=2.0):
        """world position whose projection is pixel (u, v); exact for z = 2 and (u, v) on half-integers"""
        u, v, z = (np.asarray(a, np.float64) for a in np.broadcast_arrays(u, v, z))
        W, H = self.image_width, self.image_height
        return np.stack([(u - 0.5 * (W - 1)) * z / self.f, (v - 0.5 * (H - 1)) * z / self.f, z], axis=-1).astype(F32)

    def cov(self, a, b, c, z=2.0):
        """cov3D_precomp [n,6] whose EWA projection is (a + 0.3, b, c + 0.3): the z row is zero, so J's third column drops out
        and cov2D = (f / z)^2 (c0, c1, c3) -- exact for f / z a power of two"""
        a, b, c, z = (np.asarray(x, np.float64) for x in np.broadcast_arrays(a, b, c, z))
        j2 = (self.f / z) ** 2
        out = np.zeros(a.shape + (6,), F32)
        out[..., 0], out[..., 1], out[..., 3] = a / j2, b / j2, c / j2
        return out


class Scene:
    def __init__(self, cam, xyz, op, cols, cov=None, scales=None, rots=None, bg=BG):
        self.cam, self.bg = cam, np.asarray(bg, F32)
        self.xyz = np.ascontiguousarray(np.asarray(xyz, F32).reshape(-1, 3))
        P = self.xyz.shape[0]
        self.op = np.broadcast_to(np.asarray(op, F32), (P,)).astype(F32, copy=True)
        self.cols = np.broadcast_to(np.asarray(cols, F32), (P, 3)).astype(F32, copy=True)
        self.cov = None if cov is None else np.ascontiguousarray(np.asarray(cov, F32).reshape(P, 6))
        self.scales = None if scales is None else np.broadcast_to(np.asarray(scales, F32), (P, 3)).astype(F32, copy=True)
        self.rots = None if rots is None else np.broadcast_to(np.asarray(rots, F32), (P, 4)).astype(F32, copy=True)
        self.P = P

    def kw(self):
        k = dict(colors_precomp=self.cols)
        if self.cov is not None:
            k["cov3D_precomp"] = self.cov
        else:
            k.update(scales=self.scales, rotations=self.rots)
        return k

    def keep(self, mask):
        sel = lambda a: None if a is None else a[mask]
        return Scene(self.cam, self.xyz[mask], self.op[mask], self.cols[mask], sel(self.cov), sel(self.scales), sel(self.rots), self.bg)

    @functools.cached_property
    def ref(self):
        """the oracle's record, lists and image, computed once and frozen"""
        c, W, H = self.cam, self.cam.image_width, self.cam.image_height
        geom = oracle.preprocess(self.xyz, self.scales, self.rots, self.op, None, c.world_view_transform, c.full_proj_transform,
                                 c.camera_center, W, H, c.tanfovx, c.tanfovy, cov3D_precomp=self.cov, colors_precomp=self.cols)
        pl, ranges = oracle.bin_instances(geom, W, H)
        img, final_T, n_contrib = oracle.render(W, H, ranges, pl, geom["means2D"], self.cols, geom["conic_opacity"], self.bg)
        cmax = float(max(1.0, self.cols.max(initial=0.0), self.bg.max()))
        fb = oracle.render_flip_bounds(W, H, ranges, pl, geom["means2D"], geom["conic_opacity"], cmax, rel_eps=1e-5)
        # the culled lists and the rects they are binned with: the oracle forms the cull box from the projected covariance, as the
        # kernel does, so these are exact too
        culled = {lvl: oracle.bin_instances(geom, W, H, exact_cull=lvl, want_rect=True) for lvl in (1, 2)}
        n_cull = {0: int(pl.size), 1: int(culled[1][0].size), 2: int(culled[2][0].size)}
        out = dict(geom=geom, pl=pl, ranges=ranges, img=img, final_T=final_T, n_contrib=n_contrib, n_cull=n_cull, culled=culled,
                   flips=int(((fb["n_alpha"].astype(np.int64) + fb["n_T"] + fb["n_power"]) > 0).sum()))
        for a in list(geom.values()) + [pl, ranges, img, final_T, n_contrib]:
            a.setflags(write=False)
        return out


def render(be, sc, variant=4, mode=2, rows=1, cull=0):
    c, d = sc.cam, be.dev
    r = Rasterizer(0, lib=be.lib)
    r.set_option(_lib.OPT_BLEND_VARIANT, variant)
    r.set_option(_lib.OPT_BLEND_MODE, mode)
    r.set_option(_lib.OPT_TILE_ROWS, rows)
    r.set_option(_lib.OPT_EXACT_TILE_CULL, cull)
    img, radii = r.forward(d(sc.xyz), d(sc.op), d(c.world_view_transform), d(c.full_proj_transform), d(c.camera_center), d(sc.bg),
                           c.image_width, c.image_height, c.tanfovx, c.tanfovy, **{k: d(v) for k, v in sc.kw().items()})
    return r, be.host(img), be.host(radii)


def check_record(r, radii, sc, rows):
    """cull 0: radii, rects, tile counts, the record of every visible splat and (16 x 16 lists) the instance lists: exact"""
    ref, W, H = sc.ref, sc.cam.image_width, sc.cam.image_height
    g_ref = ref["geom"]
    np.testing.assert_array_equal(radii, g_ref["radii"])
    g = r.download_geometry(0, sc.P)
    np.testing.assert_array_equal(g["rect"].astype(np.uint32), g_ref["rect"])
    np.testing.assert_array_equal(g["tiles_touched"], g_ref["tiles_touched"])
    vis = g_ref["radii"] > 0
    for k in ("means2D", "depths", "conic_opacity"):
        np.testing.assert_array_equal(g[k][vis], g_ref[k][vis], err_msg=k)
    np.testing.assert_array_equal(g["rgb"][vis], sc.cols[vis])
    if rows == 1:
        assert r.last_num_rendered == ref["pl"].size
        pl, ranges = r.download_binning(0, ref["pl"].size, ref["ranges"].shape[0])
        np.testing.assert_array_equal(ranges, ref["ranges"])
        np.testing.assert_array_equal(pl, ref["pl"])


def check_culled(r, sc, rows, cull, tag=""):
    """cull 1 / 2: the stored rects (16 x 16 units, whatever the binning tile) and, for 16 x 16 lists, num_rendered and the instance
    lists are the oracle's, exactly -- on either back-end, so the emulator and the GPU produce the same integers"""
    pl_ref, ranges_ref, rect_ref = sc.ref["culled"][cull]
    g = r.download_geometry(0, sc.P)
    np.testing.assert_array_equal(g["rect"].astype(np.uint32), rect_ref, err_msg=tag)
    if rows == 1:
        assert r.last_num_rendered == pl_ref.size, (tag, r.last_num_rendered, pl_ref.size)
        pl, ranges = r.download_binning(0, pl_ref.size, ranges_ref.shape[0])
        np.testing.assert_array_equal(ranges, ranges_ref, err_msg=tag)
        np.testing.assert_array_equal(pl, pl_ref, err_msg=tag)


def sweep(be, sc, blends=BLENDS, culls=CULLS, at_threshold=False, flips_allowed=False):
    """Every (variant, mode, rows) x cull level against the oracle.  -> {(variant, mode, rows, cull): image}.
    at_threshold: the scene puts a value ON a decision threshold: only the attributed bound applies to the image."""
    ref, W, H = sc.ref, sc.cam.image_width, sc.cam.image_height
    if not (at_threshold or flips_allowed):
        assert ref["flips"] == 0, f"the oracle finds {ref['flips']} pixels with a decision within 1e-5 of its threshold"
    imgs = {}
    for variant, mode, rows in blends:
        for cull in culls:
            r, img, radii = render(be, sc, variant, mode, rows, cull)
            tag = f"variant {variant} mode {mode} rows {rows} cull {cull}"
            np.testing.assert_array_equal(radii, ref["geom"]["radii"], err_msg=tag)
            if cull == 0:
                check_record(r, radii, sc, rows)
            else:
                check_culled(r, sc, rows, cull, tag)
            try:
                if not at_threshold:
                    assert_image_close(img, ref["img"])
                assert_image_attributed(img, ref["geom"], W, H, sc.bg, rgb=sc.cols)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            imgs[(variant, mode, rows, cull)] = img
    for (variant, mode, rows, cull), img in imgs.items():
        if not at_threshold:
            # the exact cull preserves the image; the loop forms 2 and 3 are one arithmetic (test_raster_parity states both)
            if (variant, mode, rows, 0) in imgs:
                np.testing.assert_array_equal(img, imgs[(variant, mode, rows, 0)], err_msg=f"variant {variant} mode {mode} rows {rows}: cull {cull} vs 0")
            if mode == 3 and (variant, 2, rows, cull) in imgs:
                np.testing.assert_array_equal(img, imgs[(variant, 2, rows, cull)], err_msg=f"rows {rows} cull {cull}: mode 3 vs mode 2")
    return imgs


CAM = Cam(64, 32, 64.0)          # 4 x 2 tiles; 2 f / W = 2, 2 f / H = 4, f / z = 32 at depth 2: every product below is exact
RGB = np.array([[0.9, 0.2, 0.4], [0.3, 0.8, 0.1], [0.2, 0.5, 0.95], [0.7, 0.7, 0.1], [0.1, 0.9, 0.8], [0.6, 0.1, 0.7]], F32)


def colours(n):
    return RGB[np.arange(n) % len(RGB)]


# ---- near cull --------------------------------------------------------------------------------------------------------
def near_scene():
    z = np.array([nxt(0.2, -1), F32(0.2), nxt(0.2, 1)], F32)
    xyz = np.stack([CAM.place(16 + 16 * i, 24, float(z[i])) for i in range(3)])
    xyz[:, 2] = z                                  # the view transform is the identity: t.z = z bit for bit
    sigma2 = 9.0                                   # 3 px
    cov = np.stack([CAM.cov(sigma2, 0.0, sigma2, float(z[i])) for i in range(3)])
    return Scene(CAM, xyz, 0.8, colours(3), cov=cov), z


def test_near_cull_at_its_threshold(backend):
    sc, z = near_scene()
    g = sc.ref["geom"]
    assert z[0] < F32(0.2) < z[2] and z[1] == F32(0.2)
    assert list(g["radii"] > 0) == [False, False, True] and g["depths"][2] == z[2], "t.z <= 0.2f culls, the next float does not"
    sweep(backend, sc)
    r = Rasterizer(0, lib=backend.lib)
    got = backend.host(r.mark_visible(backend.dev(sc.xyz), backend.dev(CAM.world_view_transform), backend.dev(CAM.full_proj_transform)))
    assert list(got.astype(bool)) == [False, False, True]
    np.testing.assert_array_equal(got.astype(bool), oracle.mark_visible(sc.xyz, CAM.world_view_transform, CAM.full_proj_transform))


# ---- frustum clamp ----------------------------------------------------------------------------------------------------
CLAMP_RHO = (1.29, 1.3 * (1 - REL), None, 1.3 * (1 + REL), 1.31)     # None: t.x / t.z == 1.3f tan(fov) bit for bit


def clamp_scene():
    """20 splats of sigma ~8 px at depth 2, centred rho tan(fov) z off the axis, on each axis and each sign: 9 .. 10 px outside the
    image, reaching into it.  Scales and rotations (identity), so that Sigma has a z part and J's clamped column matters."""
    xyz, side = [], []
    for axis, tan in ((0, CAM.tanfovx), (1, CAM.tanfovy)):
        lim = F32(1.3) * F32(tan)
        for sign in (1.0, -1.0):
            for k, rho in enumerate(CLAMP_RHO):
                t = lim if rho is None else F32(rho * tan)
                p = np.zeros(3, F32)
                p[axis] = F32(sign) * t * F32(2.0)             # exact: z = 2
                p[1 - axis] = F32(0.125) * (k - 2)             # spread along the border
                p[2] = 2.0
                xyz.append(p)
                ratio = p[axis] / p[2]
                assert (abs(ratio) == lim) if rho is None else ((abs(ratio) > lim) == (rho > 1.3)), (axis, sign, rho, ratio, lim)
                side.append(0 if rho is None else (1 if rho > 1.3 else -1))
    n = len(xyz)
    s = np.full((n, 3), 8.0 * 2.0 / 64.0, F32)
    s[:, 2] = 0.5
    return Scene(CAM, np.array(xyz), np.linspace(0.3, 0.9, n), colours(n), scales=s, rots=np.array([1, 0, 0, 0], F32)), np.array(side)


def test_frustum_clamp_on_each_axis_and_sign(backend):
    sc, side = clamp_scene()
    g = sc.ref["geom"]
    W, H = CAM.image_width, CAM.image_height
    m = g["means2D"]
    assert (g["radii"] > 0).all() and (side != 0).sum() == 16
    outside = (m[:, 0] < -0.5) | (m[:, 0] > W - 0.5) | (m[:, 1] < -0.5) | (m[:, 1] > H - 0.5)
    assert outside.all() and (g["tiles_touched"] > 0).all(), "off-screen but reaching into the image"
    assert np.abs(sc.ref["img"] - BG[:, None, None]).max() > 0.05, "they paint the image"
    sweep(backend, sc, flips_allowed=True)


# ---- singular and negative determinants -------------------------------------------------------------------------------
def det_f32(a, b, c):
    return F32(F32(a) * F32(c)) - F32(F32(b) * F32(b))


@functools.lru_cache(maxsize=None)
def det_search():
    """a = c = fl(8 + 0.3); b among the floats next to a: -> b with det == 0, the b with the negative det nearest to 0, the two b
    with the smallest positive dets"""
    a = F32(F32(8.0) + F32(0.3))
    cand = [(det_f32(a, nxt(a, k), a), nxt(a, k)) for k in range(-6, 7)]
    zero = [b for d, b in cand if d == 0]
    neg = sorted([(d, b) for d, b in cand if d < 0], reverse=True)
    pos = sorted([(d, b) for d, b in cand if d > 0])
    assert zero and neg and len(pos) >= 2
    return a, zero[0], neg[0][1], pos[0][1], pos[1][1]


def det_scene():
    """0: det == 0 (culled).  1: det < 0 by one rounding, centred half a pixel off the grid: its ridge d.x = d.y passes through no
    pixel centre, power <= -K / 8 everywhere.  2, 3: the two smallest positive dets, centred ON the bottom-left and the top-right
    pixel: the ridge leaves the image at once, the centre pixel has power = 0 and alpha = o.  4: det = 1.69 - 4, clearly
    negative, a saddle that contributes along its diagonal inside one tile.  5: a wide splat behind them all."""
    a, b0, bn, bp1, bp2 = det_search()
    W, H = CAM.image_width, CAM.image_height
    uv = [(30, 10), (20.5, 24), (0, H - 1), (W - 1, 0), (40, 8), (31.5, 15.5)]
    A = [8.0] * 4 + [1.0, 300.0]                    # 1024 c0 = 8 exactly, and fl(8 + 0.3f) = a
    B = [b0, bn, bp1, bp2, 2.0, 0.0]
    z = [2.0] * 5 + [4.0]
    xyz = np.stack([CAM.place(u, v, zz) for (u, v), zz in zip(uv, z)])
    cov = np.stack([CAM.cov(float(A[i]), float(B[i]), float(A[i]), z[i]) for i in range(6)])
    return Scene(CAM, xyz, [0.9, 0.9, 0.7, 0.6, 0.9, 0.5], colours(6), cov=cov)


def staging_flags(co):
    """degenerate / singular of raster_blend.h's staging step, on the record's conic (fp32, no contraction)"""
    ca, cb, cc = F32(co[0]), F32(co[1]), F32(co[2])
    det = F32(ca * cc) - F32(cb * cb)
    return (not det > 0), (not (ca > 0 and cc > 0 and det >= F32(1e-3) * ca * cc))


def test_singular_and_negative_determinants(backend):
    sc = det_scene()
    ref = sc.ref
    g = ref["geom"]
    a = det_search()[0]
    # cov2D as the kernel forms it: 1024 c0 + 0.3
    for i in range(4):
        assert F32(F32(1024.0) * sc.cov[i, 0]) + F32(0.3) == a, "the 3D entry does not project to a"
    assert g["radii"][0] == 0 and g["tiles_touched"][0] == 0, "det == 0 is culled"
    assert (g["radii"][1:] > 0).all() and (g["tiles_touched"][1:] > 0).all(), "det < 0 and the smallest det > 0 are instances"
    alone = sc.keep(np.arange(6) == 1)
    assert (alone.ref["n_contrib"] == 0).all() and alone.ref["pl"].size > 0, "det < 0 by a rounding: instances that contribute nowhere"
    for i in (2, 3):
        assert staging_flags(g["conic_opacity"][i])[1], "the smallest positive dets take the singular (general) path"
        one = sc.keep(np.arange(6) == i).ref
        assert (one["n_contrib"] > 0).sum() == 1, "only the centre pixel"
    assert staging_flags(g["conic_opacity"][4]) == (True, True) and g["conic_opacity"][4][0] < 0
    saddle = sc.keep(np.arange(6) == 4).ref
    assert (saddle["n_contrib"] > 0).sum() >= 9 and (saddle["n_contrib"][:16, 32:48] > 0).sum() == (saddle["n_contrib"] > 0).sum()
    imgs = sweep(backend, sc)
    # one image, whatever the tile height
    for (variant, mode, rows, cull), img in imgs.items():
        if rows == 2:
            np.testing.assert_array_equal(img, imgs[(variant, mode, 1, cull)])


# ---- rect arithmetic --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def radius_search():
    """cov entries (a - 0.3 as passed to Cam.cov, in units of 1 / 1024) whose 3 sqrt(lambda) is EXACTLY 6 and the next float above
    6: radius 6 and 7.  The chain is project_view's, in fp32: a = 1024 c0 + 0.3, lambda = a + sqrt(max(0.1, a a - a a))."""
    def three_sqrt(c0):
        a = F32(F32(1024.0) * c0) + F32(0.3)
        mid = F32(0.5) * F32(a + a)
        det = F32(a * a)
        lam = mid + np.sqrt(np.maximum(F32(0.1), F32(mid * mid) - det))
        return F32(3.0) * np.sqrt(lam)
    c0 = F32((4.0 - 0.3 - np.sqrt(0.1)) / 1024.0)
    exact = above = None
    for k in range(-64, 65):
        t = three_sqrt(nxt(c0, k))
        if t == F32(6.0):
            exact = nxt(c0, k)
        if t > F32(6.0) and above is None:
            above = nxt(c0, k)
            assert F32(6.0) < t <= nxt(6.0, 2), "the first value above 6"
    assert exact is not None and above is not None
    return exact, above


def rect_scene(cam, centres, c0=None):
    c0 = radius_search()[0] if c0 is None else c0
    n = len(centres)
    xyz = np.stack([cam.place(u, v) for u, v in centres])
    cov = np.zeros((n, 6), F32)
    cov[:, 0] = cov[:, 3] = c0
    return Scene(cam, xyz, np.linspace(0.3, 0.8, n), colours(n), cov=cov)


RECT_BLENDS = [(0, 2, 1), (4, 2, 1), (4, 2, 2)]


def test_radius_at_an_exact_integer_and_one_ulp_above(backend):
    exact, above = radius_search()
    sc = rect_scene(CAM, [(20, 20), (44, 20)])
    sc.cov[1, 0] = sc.cov[1, 3] = above
    g = sc.ref["geom"]
    assert list(g["radii"]) == [6, 7]
    sweep(backend, sc, RECT_BLENDS)


def test_rect_casts_and_the_zero_area_test(backend):
    """radius 6 on a 64 x 32 image (4 x 2 tiles).  (x0, y0, x1, y1) written out per centre."""
    cases = [((3, 20), (0, 0, 1, 2)),          # mx - r = -3: truncates toward zero to tile 0
             ((6, 20), (0, 0, 1, 2)),          # mx - r = 0; mx + r + 15 = 27
             ((11, 8), (0, 0, 2, 1)),          # mx + r + 15 = 32, a multiple of 16: x1 = 2; my + r + 15 = 29: y1 = 1
             ((10, 8), (0, 0, 1, 1)),          # 31 / 16: x1 = 1 -- exactly one tile
             ((22, 22), (1, 1, 2, 2)),         # mx - r = 16: x0 = 1; 43 / 16: x1 = 2
             ((-6, 8), (0, 0, 0, 0)),          # left of the image: mx + r + 15 = 15: empty
             ((-5, 8), (0, 0, 1, 1)),          # ... 16: one tile
             ((70, 8), (0, 0, 0, 0)),          # right: mx - r = 64 = 4 tiles: x0 = gx: empty
             ((69.5, 8), (3, 0, 4, 1)),        # 63.5 / 16: x0 = 3
             ((8, -6), (0, 0, 0, 0)),          # above
             ((8, -5), (0, 0, 1, 1)),
             ((8, 38), (0, 0, 0, 0)),          # below: my - r = 32 = 2 tiles
             ((8, 37.5), (0, 1, 1, 2)),
             ((-5, -5), (0, 0, 1, 1)),         # the corners: one tile
             ((69.5, 37.5), (3, 1, 4, 2)),
             ((-6, -5), (0, 0, 0, 0)), ((70, 37.5), (0, 0, 0, 0))]
    sc = rect_scene(CAM, [c for c, _ in cases])
    g = sc.ref["geom"]
    np.testing.assert_array_equal(g["rect"], np.array([r for _, r in cases], np.uint32))
    np.testing.assert_array_equal(g["radii"], [6 if r[2] else 0 for _, r in cases])
    vis = g["radii"] > 0
    np.testing.assert_array_equal(g["means2D"][vis], np.array([c for c, _ in cases], F32)[vis])    # the centres are exact
    sweep(backend, sc, RECT_BLENDS)


@pytest.mark.parametrize("W", [1, 15, 16, 17, 33])
def test_image_sizes_around_one_tile(backend, W):
    """W, H in {1, 15, 16, 17, 33}: partial tiles, one tile exactly, one pixel more; H = 1 .. 16 and H = 33 have an odd number of
    tile rows under 16 x 32 binning tiles.  Splats on the corners, on the last pixel, one pixel outside and far outside."""
    for H in (1, 15, 16, 17, 33):
        cam = Cam(W, H, 64.0)
        centres = [(0, 0), (W - 1, H - 1), (W, H), (W - 1, 0), (0.5 * (W - 1), 0.5 * (H - 1)), (-6, 0), (-5, 0), (W + 5, H - 1),
                   (W + 4.5, H - 1), (0, H + 5), (0, H + 4.5), (16, 16), (15.5, 15.5), (W + 40, 0), (0, H + 40), (-40, -40)]
        sc = rect_scene(cam, centres)
        g = sc.ref["geom"]
        assert g["radii"][0] == 6 and (g["radii"][-3:] == 0).all()
        sweep(backend, sc, RECT_BLENDS, flips_allowed=True)


# ---- opacity floor ----------------------------------------------------------------------------------------------------
def dots(ops, cam=CAM):
    """one splat of sigma ~1.5 px per opacity, each centred on a pixel centre of its own tile: power = 0 there, alpha = o"""
    n = len(ops)
    centres = [(8 + 16 * (i % 4), 8 + 16 * (i // 4)) for i in range(n)]
    xyz = np.stack([cam.place(u, v) for u, v in centres])
    return Scene(cam, xyz, np.array(ops, F32), colours(n), cov=cam.cov(2.0, 0.0, 2.0)[None].repeat(n, 0)), centres


def test_opacity_floor_side_points(backend):
    ops = [F32(0.0), F32(THR * F32(1 - REL)), F32(THR * F32(1 + REL)), F32(0.5)]
    sc, centres = dots(ops)
    ref = sc.ref
    assert ops[1] < THR < ops[2] and (ref["geom"]["radii"] > 0).all()
    n = ref["n_contrib"]
    assert [int(n[v, u]) for u, v in centres] == [0, 0, 1, 1], "alpha = o: below the floor skips, above contributes"
    assert ref["n_cull"][1] == 2 and ref["n_cull"][0] == 4, "thr < 0 empties the rect of the two splats under the floor"
    sweep(backend, sc)


def test_opacity_floor_at_the_value(backend):
    sc, centres = dots([THR, F32(0.5)])
    ref = sc.ref
    (u, v) = centres[0]
    assert ref["n_contrib"][v, u] == 1 and ref["flips"] >= 1, "alpha == 1/255 is not < 1/255: it contributes, and the oracle flags it"
    assert F32(THR * F32(255.0)) >= 1, "the cull threshold keeps it"
    imgs = sweep(backend, sc, at_threshold=True)
    # variant 0 forms alpha = o * exp(0) = o: the reference's decision, not a flip
    for cull in CULLS:
        np.testing.assert_allclose(imgs[(0, 2, 1, cull)][:, v, u], ref["img"][:, v, u], rtol=0, atol=CLEAN_BAR)


# ---- alpha cap --------------------------------------------------------------------------------------------------------
CAP_OPS = [F32(0.98), nxt(0.98, 1), F32(F32(0.99) * F32(1 - REL)), nxt(0.99, -1), F32(0.99), F32(F32(0.99) * F32(1 + REL)), F32(1.0), F32(0.97)]


def test_alpha_cap(backend):
    sc, centres = dots(CAP_OPS)
    ref = sc.ref
    assert (ref["geom"]["conic_opacity"][1:7, 3] > F32(0.98)).all() and ref["geom"]["conic_opacity"][0, 3] == F32(0.98)
    for i, (u, v) in enumerate(centres):
        al = np.minimum(F32(0.99), CAP_OPS[i])
        want = sc.cols[i] * al * F32(1.0) + F32(F32(1.0) - al) * BG          # known answer on the centre pixel
        np.testing.assert_array_equal(ref["img"][:, v, u], want)
        if CAP_OPS[i] > F32(0.99):
            np.testing.assert_array_equal(want, sc.cols[i] * F32(0.99) + F32(F32(1.0) - F32(0.99)) * BG)
    imgs = sweep(backend, sc)
    for key, img in imgs.items():
        for i, (u, v) in enumerate(centres):
            np.testing.assert_allclose(img[:, v, u], ref["img"][:, v, u], rtol=0, atol=CLEAN_BAR, err_msg=f"{key} opacity {CAP_OPS[i]}")


def test_capped_instances_at_the_ends_of_a_staged_batch(backend):
    """130 splats of sigma 6 px on one pixel centre, opacity 0.02 but for 0.995 at list positions 0, 31, 63 (first, middle and last
    slot of the first 64-instance batch) ... each in a scene of its own, and 64 (slot 0 of the second batch)."""
    for pos in (0, 31, 63, 64):
        n = 130
        xyz = np.repeat(CAM.place(24, 24)[None], n, 0)
        xyz[:, 2] = 2.0 + np.arange(n) * 2.0 ** -10                 # list order = index
        xyz[:, :2] *= (xyz[:, 2:3] / 2.0)                           # all on pixel (24, 24)
        op = np.full(n, 0.02, F32)
        op[pos] = 0.995
        cov = np.stack([CAM.cov(36.0, 0.0, 36.0, float(z)) for z in xyz[:, 2]])
        sc = Scene(CAM, xyz, op, colours(n), cov=cov)
        ref = sc.ref
        t = ref["ranges"][1 * 4 + 1]
        assert list(ref["pl"][t[0]:t[1]]) == list(range(n)) and ref["geom"]["conic_opacity"][pos, 3] > F32(0.98)
        sweep(backend, sc, flips_allowed=True)


def test_several_capped_instances_in_one_staged_batch(backend):
    """One list of 70 instances in tile (1, 1): 66 splats of opacity 0.02 stacked on pixel (24, 24), and capped ones (opacity
    0.995, sigma 1 px, each on a pixel centre of its own so that no pixel saturates) at list positions 0, 31, 63 -- the first, a
    middle and the last slot of the first 64-instance batch: three general-path slots, several run splits -- and 64, slot 0 of
    the second batch."""
    n, capped = 70, {0: (18, 18), 31: (29, 19), 63: (19, 29), 64: (29, 29)}
    uv = np.array([capped.get(i, (24, 24)) for i in range(n)], np.float64)
    z = 2.0 + np.arange(n) * 2.0 ** -10                              # list order = index
    xyz = CAM.place(uv[:, 0], uv[:, 1], z)
    op = np.array([0.995 if i in capped else 0.02 for i in range(n)], F32)
    var = np.array([1.0 if i in capped else 36.0 for i in range(n)])
    sc = Scene(CAM, xyz, op, colours(n), cov=CAM.cov(var, 0.0, var, z))
    ref = sc.ref
    t = ref["ranges"][1 * 4 + 1]
    assert list(ref["pl"][t[0]:t[1]]) == list(range(n)) and (ref["geom"]["conic_opacity"][list(capped), 3] > F32(0.98)).all()
    for i, (u, v) in capped.items():
        assert ref["final_T"][v, u] < 0.011 and ref["n_contrib"][v, u] > i, "the capped splat contributes with alpha 0.99"
    sweep(backend, sc, flips_allowed=True)


# ---- saturation -------------------------------------------------------------------------------------------------------
# the splats of a stack have no red: the red channel reads out T, out = 0 + T bg, to fp32's RELATIVE precision


def stack(ops, cam=CAM):
    n = len(ops)
    xyz = np.repeat(cam.place(24, 24)[None], n, 0)
    xyz[:, 2] = 2.0 + np.arange(n) * 2.0 ** -10
    xyz[:, :2] *= (xyz[:, 2:3] / 2.0)
    cov = np.stack([cam.cov(4.0, 0.0, 4.0, float(z)) for z in xyz[:, 2]])
    cols = colours(n).copy()
    cols[:, 0] = 0.0
    return Scene(cam, xyz, np.array(ops, F32), cols, cov=cov)


def contributions(img, alpha, u=24, v=24):
    """number of accumulated contributions on the pixel, from T = red / bg = (1 - alpha)^n"""
    return int(np.rint(np.log(float(img[0, v, u]) / float(BG[0])) / np.log1p(-float(alpha))))


@pytest.mark.parametrize("alpha,n", [(0.99, 4), (0.9, 8), (0.5, 20), (0.1325, 70)])
def test_saturation_stops_where_the_reference_stops(backend, alpha, n):
    """identical splats on a pixel centre: T = (1 - alpha)^k.  0.99: 1, 0.01, then 0.01^2 < 0.0001f stops.  0.1325: T_64 = 1.12e-4,
    T_65 = 9.7e-5: the instance that saturates is slot 0 of the second 64-instance batch."""
    sc = stack([alpha] * n)
    ref = sc.ref
    count = int(ref["n_contrib"][24, 24])
    assert 0 < count < n - 1 and contributions(ref["img"], F32(alpha)) == count, "the stack saturates before its end"
    if alpha == 0.5:
        assert count == 13          # 2^-13 >= 1e-4 > 2^-14, in any arithmetic
    if alpha == 0.1325:
        assert count == 64          # the 65th instance, slot 0 of the second batch, saturates
    imgs = sweep(backend, sc, flips_allowed=True)
    for key, img in imgs.items():
        assert contributions(img, F32(alpha)) == count, key


@functools.lru_cache(maxsize=None)
def t_search():
    """opacities (o1, 0.995 -> alpha 0.99, o3) with fl(fl(fl(1 - o1) * fl(1 - 0.99f)) * fl(1 - o3)) == 0.0001f bit for bit"""
    target = F32(0.0001)
    m = F32(1.0) - F32(0.99)
    for k in range(4000):
        o1 = nxt(0.9, 0) + F32(k) * F32(2.0 ** -20)
        t2 = F32(F32(F32(1.0) - o1) * m)
        o3 = F32(1.0) - F32(target / t2)
        for j in range(-3, 4):
            o = nxt(o3, j)
            if F32(t2 * F32(F32(1.0) - o)) == target and o < F32(0.98):
                return o1, F32(0.995), o
    raise AssertionError("no stack found")


def test_saturation_at_the_value(backend):
    """T' == 0.0001f is not < 0.0001f: the third splat contributes.  Variant 0 forms T (1 - alpha) literally and must do so too."""
    ops = list(t_search()) + [F32(0.5)]
    sc = stack(ops)
    ref = sc.ref
    assert ref["final_T"][24, 24] == F32(0.0001) and ref["n_contrib"][24, 24] == 3 and ref["flips"] >= 1
    imgs = sweep(backend, sc, at_threshold=True)
    for cull in CULLS:
        np.testing.assert_allclose(imgs[(0, 2, 1, cull)][:, 24, 24], ref["img"][:, 24, 24], rtol=0, atol=CLEAN_BAR)


# ---- quantisation -----------------------------------------------------------------------------------------------------
def tie(k):
    """bg with fl(bg * 255) == k + 0.5"""
    b = F32((k + 0.5) / 255.0)
    for j in range(-3, 4):
        if F32(nxt(b, j) * F32(255.0)) == F32(k + 0.5):
            return nxt(b, j)
    raise AssertionError(k)


def views(be, xyz, op, rgb, bg, s=0.05, cam=CAM):
    P = len(xyz)
    shs = np.zeros((P, 1, 3), F32)
    shs[:, 0] = RGB2SH(np.asarray(rgb, np.float64))
    gd = dict(xyz=be.dev(np.ascontiguousarray(xyz, F32)), scaling=be.dev(np.full((P, 3), s, F32)),
              rotation=be.dev(np.tile(np.array([1, 0, 0, 0], F32), (P, 1))), opacity=be.dev(np.ascontiguousarray(op, F32)),
              features=be.dev(shs), raw=False, sh_degree=0)
    c = make_camera(cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy, cam.world_view_transform, cam.full_proj_transform,
                    cam.camera_center)
    r = Rasterizer(0, lib=be.lib)
    res = r.render_views(gd, [c], bg=tuple(float(b) for b in bg), want_rgb8=True)
    return be.host(res["color"])[0], be.host(res["rgb8"])[0]


def test_quantisation_ties_and_clamps(backend):
    vals = [tie(100), tie(101), tie(0), tie(254), F32(-0.25), F32(1.5), F32(-0.0), nxt(1.0, -1), nxt(1.0, 1), F32(0.0), F32(1.0), tie(37)]
    assert F32(vals[0] * F32(255.0)) == F32(100.5) and F32(vals[1] * F32(255.0)) == F32(101.5)
    behind = np.array([[0, 0, -5.0]], F32)
    for i in range(0, len(vals), 3):
        bg = np.array(vals[i:i + 3], F32)
        color, rgb8 = views(backend, behind, [0.5], [[0.5, 0.5, 0.5]], bg)
        want = np.clip(np.rint(bg * F32(255.0)), 0, 255).astype(np.uint8)
        np.testing.assert_array_equal(color, np.broadcast_to(bg[:, None, None], color.shape))
        np.testing.assert_array_equal(rgb8, np.broadcast_to(want, rgb8.shape), err_msg=str(bg))
    assert list(np.clip(np.rint(np.array(vals[:2], F32) * F32(255.0)), 0, 255)) == [100, 102], "half to even"


def test_rgb8_is_the_quantised_colour_on_a_capped_centre(backend):
    color, rgb8 = views(backend, CAM.place([24, 40], [24, 24]), [1.0, 0.6], [[0.9, 0.2, 0.4], [0.3, 0.8, 0.1]], BG, s=0.1)
    want = F32(0.9) * F32(0.99) + F32(F32(1.0) - F32(0.99)) * BG[0]
    assert abs(color[0, 24, 24] - want) <= CLEAN_BAR
    np.testing.assert_array_equal(rgb8, np.clip(np.rint(color.transpose(1, 2, 0) * F32(255.0)), 0, 255).astype(np.uint8))


# ---- non-finite and overflowing splats (DESIGN.md "Parity") ----------------------------------------------------------
NAN, INF = F32(np.nan), F32(np.inf)
BAD_KINDS = ["scale nan", "scale inf", "rot nan", "x nan", "y nan", "z nan", "x inf", "y -inf", "z inf", "op nan", "op inf", "op -inf"]


def ordinary(n=200, seed=7):
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 4.0, n)
    xyz = CAM.place(rng.uniform(-4, 68, n), rng.uniform(-4, 36, n), z)
    s = (rng.uniform(1.0, 6.0, (n, 3)) * z[:, None] / 64.0).astype(F32)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    return xyz, s, q, rng.uniform(0.05, 0.95, n).astype(F32), rng.uniform(0, 1, (n, 3)).astype(F32)


def spoil(kind, xyz, s, q, o, cov=None):
    what, val = kind.split()
    val = {"nan": NAN, "inf": INF, "-inf": -INF, "1e18": F32(1e18)}[val]
    if what == "scale":
        if cov is None:
            s[1] = val
        else:
            cov[3] = val * val if np.isfinite(val) else val
    elif what == "rot":
        if cov is None:
            q[2] = val
        else:
            cov[1] = val
    elif what in "xyz":
        xyz["xyz".index(what)] = val
    else:
        o[()] = val


@functools.lru_cache(maxsize=None)
def bad_scene(precomp, kinds=tuple(BAD_KINDS)):
    """200 ordinary splats + one bad splat of each kind twice: centred in tile (0, 0) and in the interior (the level-1 cull's box
    of a NaN extent is tile column / row 0).  -> (scene, mask of the bad ones)"""
    xyz, s, q, o, cols = ordinary()
    bx, bs, bq, bo = [], [], [], []
    for u, v in ((5, 6), (40, 24)):
        for kind in kinds:
            bx.append(CAM.place(u, v, 2.5)), bs.append(np.full(3, 0.05, F32)), bq.append(np.array([1, 0, 0, 0], F32)), bo.append(F32(0.7))
    nb = len(bx)
    X, S, Q, O = np.concatenate([xyz, np.array(bx)]), np.concatenate([s, np.array(bs)]), np.concatenate([q, np.array(bq)]), \
        np.concatenate([o, np.array(bo)])
    C = np.concatenate([cols, np.tile(np.array([[1.0, 0.0, 1.0]], F32), (nb, 1))])
    n = len(xyz)
    cov = None
    if precomp:
        cov = oracle.preprocess(X, S, Q, O, None, CAM.world_view_transform, CAM.full_proj_transform, CAM.camera_center, 64, 32,
                                CAM.tanfovx, CAM.tanfovy, colors_precomp=C)["cov3D"].copy()
        cov[n:] = np.array([0.05 ** 2, 0, 0, 0.05 ** 2, 0, 0.05 ** 2], F32)
    for i in range(nb):
        spoil(kinds[i % len(kinds)], X[n + i], S[n + i], Q[n + i], O[n + i:n + i + 1].reshape(()), None if cov is None else cov[n + i])
    bad = np.arange(n + nb) >= n
    sc = Scene(CAM, X, O, C, cov=cov, scales=None if precomp else S, rots=None if precomp else Q)
    return sc, bad


def rect_mask(rects, W, H):
    """pixels inside any of the 16 x 16 tile rects"""
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in rects.astype(np.int64):
        m[16 * y0:16 * y1, 16 * x0:16 * x1] = True
    return m


def check_contract(be, sc, bad):
    W, H, gx, gy = 64, 32, 4, 2
    g_ref = sc.ref["geom"]
    clean = sc.keep(~bad)
    inside = rect_mask(g_ref["rect"][bad], W, H)
    for variant, mode, rows in BLENDS:
        for cull in CULLS:
            tag = f"variant {variant} mode {mode} rows {rows} cull {cull}"
            r, img, radii = render(be, sc, variant, mode, rows, cull)
            n = r.last_num_rendered
            g = r.download_geometry(0, sc.P)
            rect = g["rect"].astype(np.int64)
            # (a) the integers are the oracle's
            np.testing.assert_array_equal(radii, g_ref["radii"], err_msg=tag)
            if cull == 0:
                np.testing.assert_array_equal(rect, g_ref["rect"], err_msg=tag)
                np.testing.assert_array_equal(g["tiles_touched"], g_ref["tiles_touched"], err_msg=tag)
                if rows == 1:
                    assert n == sc.ref["pl"].size, tag
                    pl, ranges = r.download_binning(0, n, gx * gy)
                    np.testing.assert_array_equal(ranges, sc.ref["ranges"], err_msg=tag)
                    np.testing.assert_array_equal(pl, sc.ref["pl"], err_msg=tag)
            else:
                check_culled(r, sc, rows, cull, tag)
            # (b) every stored rect is all zero or a proper rect of the grid; the lists hold num_rendered instances, at most the rects' tiles
            zero = (rect == 0).all(axis=1)
            ok = (0 <= rect[:, 0]) & (rect[:, 0] < rect[:, 2]) & (rect[:, 2] <= gx) & (0 <= rect[:, 1]) & (rect[:, 1] < rect[:, 3]) & (rect[:, 3] <= gy)
            assert (zero | ok).all(), (tag, rect[~(zero | ok)])
            assert (rect[:, 2] <= g_ref["rect"][:, 2]).all() and (rect[:, 0] >= np.where(zero, 0, g_ref["rect"][:, 0])).all(), tag
            n_tiles = gx * ((gy + rows - 1) // rows)
            pl, ranges = r.download_binning(0, n, n_tiles)
            assert int((ranges[:, 1].astype(np.int64) - ranges[:, 0]).sum()) == n, tag
            area = ((rect[:, 2] - rect[:, 0]) * ((rect[:, 3] + rows - 1) // rows - rect[:, 1] // rows)).sum()
            assert n == area if cull == 0 else n <= area, (tag, n, area)
            # (c) outside the reference rects of the bad splats: the image of the scene without them, bit for bit
            _, img_clean, _ = render(be, clean, variant, mode, rows, cull)
            for ch in range(3):
                np.testing.assert_array_equal(img[ch][~inside], img_clean[ch][~inside], err_msg=tag)
    return inside


@pytest.mark.parametrize("precomp", [False, True])
def test_bad_splats_leave_the_rest_of_the_image_alone(backend, precomp):
    sc, bad = bad_scene(precomp)
    g = sc.ref["geom"]
    assert np.isfinite(g["radii"]).all() and (g["radii"] >= 0).all(), "no INT_MIN radius"
    t = g["tiles_touched"].astype(np.int64)
    r = g["rect"].astype(np.int64)
    np.testing.assert_array_equal(t, (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]))
    assert ((g["radii"] > 0) == (t > 0)).all(), "radius 0 <=> no tiles"
    # NaN geometry is invisible; a NaN / inf opacity keeps its finite rect
    kinds = BAD_KINDS * 2
    for i, k in enumerate(kinds):
        vis = g["radii"][200 + i] > 0
        assert vis == k.startswith("op"), (k, g["radii"][200 + i])
    inside = check_contract(backend, sc, bad)
    assert 0 < inside.sum() < inside.size / 2, "the contract is checked on most of the image"


@pytest.mark.parametrize("precomp", [False, True])
def test_a_radius_beyond_int_covers_the_grid(backend, precomp):
    """scale 1e18: 3 sqrt(lambda) is beyond INT_MAX (or inf): radius INT_MAX, the whole grid, on both back-ends and the oracle"""
    sc, bad = bad_scene(precomp, ("scale 1e18",))
    g = sc.ref["geom"]
    assert list(g["radii"][bad]) == [2 ** 31 - 1] * 2 and (g["rect"][bad] == [0, 0, 4, 2]).all() and (g["tiles_touched"][bad] == 8).all()
    for lvl in (1, 2):         # the cull box of an infinite extent: the covariance's, not NaN -- the splat keeps tiles
        assert (sc.ref["culled"][lvl][2][bad, 2] > 0).all()
    check_contract(backend, sc, bad)


def test_rgb8_of_a_nan_pixel_is_zero(backend):
    behind = np.array([[0, 0, -5.0]], F32)
    color, rgb8 = views(backend, behind, [0.5], [[0.5, 0.5, 0.5]], np.array([np.nan, 0.25, np.inf], F32))
    assert np.isnan(color[0]).all()
    np.testing.assert_array_equal(rgb8, np.broadcast_to(np.array([0, 64, 255], np.uint8), rgb8.shape))


# ---- the stand-alone program -----------------------------------------------------------------------------------------
def test_nonfinite_check_program():
    """tests/emu/raster_nonfinite_check.cpp: the bad-splat scene through gs2m_rasterize_forward at cull levels 0, 1 and 2, linked
    against the emulator objects.  (The same program is what a sanitizer build runs.)"""
    import build_emu
    build_emu.build()
    emu = os.path.dirname(os.path.abspath(build_emu.__file__))
    root = os.path.dirname(os.path.dirname(emu))
    exe = os.path.join(build_emu.OUT, "raster_nonfinite_check")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                         os.path.join(emu, "raster_nonfinite_check.cpp"), "-o", exe, "-L", build_emu.OUT, "-lgs2mesh_emu",
                         "-Wl,-rpath," + build_emu.OUT, "-fopenmp"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout
