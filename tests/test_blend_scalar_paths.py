"""The control flow of the compositing loop forms 2 and 3 (raster_blend.h), at the smallest shapes where it can go wrong.

One (instance, quadrant) of those loops is a hand-lowered block (gs2m_blend_quadrant, platform.h): a skip branch on the candidate
mask, the execution mask narrowed without a second branch, the saturation fix-up out of line, and a two-instance loop with one
back edge.  Loop form 0 (lane masks in scalar registers, compiler-lowered) and blend variant 0 (one pixel per lane, the
reference's structure) share none of that and are the yardsticks:

  * forms 2 and 3 equal form 0 BIT FOR BIT, float image and u8 image, for 16 x 16 and 16 x 32 binning tiles;
  * they equal variant 0 under assert_image_close, the bar tests/test_raster_forward_edges.py holds every kernel to.

Hand-built splats through Rasterizer.render_views on 32 x 32 (2 x 2 tiles) and 40 x 24 (partial tiles on the right and at the
bottom).  Lane l of a tile's wave owns pixel (l & 7, l >> 3) of each 8 x 8 quadrant: lane 0 its top-left, lane 63 its
bottom-right pixel.  A splat of sigma s px is centred ON a pixel centre; the 0.3 px^2 low-pass makes a "point" splat
(s = 0.3) fall to 0.28 of its peak one pixel away, so with opacity 0.008 only its own pixel reaches alpha >= 1 / 255.
"""
import functools

import numpy as np
import pytest

from gs2mesh_amd import _lib
from gs2mesh_amd.rasterizer import Rasterizer, make_camera
from gs2mesh_amd.sh_utils import RGB2SH
from test_raster_forward_edges import Cam, colours
from test_raster_parity import assert_image_close

F32 = np.float32
BG = (0.1, 0.2, 0.3)
F = 64.0                                   # focal length: 32 px per world unit at depth 2
CAM32, CAM40 = Cam(32, 32, F), Cam(40, 24, F)
Q45 = (float(np.cos(np.pi / 8)), 0.0, 0.0, float(np.sin(np.pi / 8)))       # 45 degrees about the view axis
MODES, ROWS = (0, 2, 3), (1, 2)


class Splats:
    """list order = order of the add() calls (depth grows by 2^-10 per splat; centres and sizes are rescaled to stay put)"""

    def __init__(self, cam):
        self.cam, self.rows = cam, []

    def add(self, u, v, sigma, op, rgb=None, sigma2=None, rot=(1.0, 0.0, 0.0, 0.0), n=1):
        for _ in range(n):
            i = len(self.rows)
            z = 2.0 + i * 2.0 ** -10
            c = colours(i + 1)[i] if rgb is None else np.asarray(rgb, F32)
            s2 = sigma if sigma2 is None else sigma2
            self.rows.append((self.cam.place(u, v, z), (sigma * z / F, s2 * z / F, 1e-4), rot, op, c))
        return self

    def gaussians(self, be):
        xyz, s, q, o, c = (np.array([r[k] for r in self.rows], F32) for k in range(5))
        shs = np.zeros((len(self.rows), 1, 3), F32)
        shs[:, 0] = RGB2SH(c.astype(np.float64))
        return dict(xyz=be.dev(xyz), scaling=be.dev(s), rotation=be.dev(q), opacity=be.dev(o), features=be.dev(shs), raw=False,
                    sh_degree=0)


@functools.lru_cache(maxsize=None)
def handle(be_name, lib, variant, mode, rows):
    r = Rasterizer(0, lib=lib)
    r.set_option(_lib.OPT_BLEND_VARIANT, variant)
    r.set_option(_lib.OPT_BLEND_MODE, mode)
    r.set_option(_lib.OPT_TILE_ROWS, rows)
    return r


def render(be, sp, variant, mode, rows):
    cam = sp.cam
    c = make_camera(cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy, cam.world_view_transform, cam.full_proj_transform,
                    cam.camera_center)
    res = handle(be.name, be.lib, variant, mode, rows).render_views(sp.gaussians(be), [c], bg=BG, want_rgb8=True)
    return be.host(res["color"])[0].copy(), be.host(res["rgb8"])[0].copy()


def check(be, sp, nan_ok=False, form=0):
    """forms 2, 3 == form 0 bit for bit (float, u8) for rows 1, 2; all of them close to variant 0.  -> the float image of `form`
    (16 x 16 lists).  nan_ok: the scene has a NaN colour.  Variant 0 and the forms 2 / 3 confine it to the candidate pixels
    (execution mask); form 0 masks by arithmetic (w = 0 on the other lanes of a contributing quadrant, and NaN * 0 = NaN), so
    there the forms are compared where form 0 is finite and the NaN pixels of 2 / 3 must be variant 0's exactly."""
    ref0, _ = render(be, sp, 0, 2, 1)
    bad = np.isnan(ref0)
    assert nan_ok or not bad.any()
    out = None
    for rows in ROWS:
        img0, u80 = render(be, sp, 4, 0, rows)
        ok0 = ~np.isnan(img0)
        assert (~ok0 | ~bad).all() if nan_ok else ok0.all(), "form 0 is NaN where variant 0 is, and nowhere without a NaN colour"
        for mode in MODES:
            img, u8 = (img0, u80) if mode == 0 else render(be, sp, 4, mode, rows)
            tag = f"mode {mode} rows {rows}"
            if mode != 0:
                np.testing.assert_array_equal(np.isnan(img), bad, err_msg=f"{tag}: the NaN pixels are variant 0's")
                np.testing.assert_array_equal(img[ok0], img0[ok0], err_msg=f"{tag} vs mode 0: float image")
                ok8 = ok0.all(axis=0)                                            # u8 is H x W x 3
                np.testing.assert_array_equal(u8[ok8], u80[ok8], err_msg=f"{tag} vs mode 0: u8 image")
            try:
                fin = ~np.isnan(img)
                assert_image_close(np.where(fin, img, F32(0)), np.where(fin, ref0, F32(0)))
            except AssertionError as e:
                raise AssertionError(f"{tag} vs variant 0: {e}") from None
            if mode == form and rows == 1:
                out = img
    return out


def painted(img):
    """pixels that differ from the background (H x W bool)"""
    return (img != np.array(BG, F32)[:, None, None]).any(axis=0)


# ---- run lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 129])
def test_run_lengths(backend, n):
    """n instances of sigma 2 px on pixel (7, 7): the rect is tile (0, 0) alone, every instance is staged, none is flagged, no
    pixel saturates (0.98^129 = 0.07): one run of n -- the pairs of the pipelined loop, its odd tail, its single back edge;
    63 | 64 | 65 | 129 = around one staged batch and into a third (the record prefetch stages).  With 16 x 32 lists the lower
    half of the list drops every instance while staging."""
    sp = Splats(CAM32).add(7, 7, 2.0, 0.02, n=n)
    img = check(backend, sp)
    p = painted(img)
    assert p[:16, :16].sum() > 30 and p.sum() == p[:16, :16].sum(), "tile (0, 0) and nothing else"
    # T on the centre pixel = 0.98^n to fp32 precision: every instance was composited exactly once
    want = sum(float(colours(i + 1)[i][0]) * 0.02 * 0.98 ** i for i in range(n)) + 0.98 ** n * BG[0]
    assert abs(float(img[0, 7, 7]) - want) < 2e-5 * max(1, n / 8), (float(img[0, 7, 7]), want)


# ---- candidate masks ------------------------------------------------------------------------------------------------------
POINT = dict(sigma=0.3, op=0.008)          # reaches alpha >= 1 / 255 on its own pixel only


@pytest.mark.parametrize("lane", [0, 63])
def test_a_single_candidate_lane_per_quadrant(backend, lane):
    """one point splat on the top-left (lane 0) or bottom-right (lane 63) pixel of each quadrant of tile (1, 0) and of quadrant 2
    of tile (0, 1): in its quadrant the candidate mask has that one bit, the other three quadrants of the instance have none."""
    off = 0 if lane == 0 else 7
    px = [(16 + 8 * (k & 1) + off, 8 * (k >> 1) + off) for k in range(4)] + [(off, 16 + 8 + off)]
    sp = Splats(CAM32)
    for u, v in px:
        sp.add(u, v, **POINT)
    p = painted(check(backend, sp))
    assert sorted(zip(*np.nonzero(p.T))) == sorted(px), "each splat paints its own pixel and no other"


def test_no_candidate_and_all_four_quadrants(backend):
    """a point splat centred BETWEEN four pixels of tile (0, 0) with opacity 0.007: its box reaches the quadrant, so it is staged, and
    no pixel is a candidate in any quadrant (alpha = 0.007 * 0.53 < 1 / 255) -- first, in the middle and last in the list;
    between them two splats of sigma 6 px on the tile's centre: candidates in all four quadrants."""
    sp = Splats(CAM32).add(3.5, 3.5, 0.3, 0.007).add(7.5, 7.5, 6.0, 0.6).add(11.5, 3.5, 0.3, 0.007).add(7.5, 7.5, 6.0, 0.5)
    sp.add(3.5, 11.5, 0.3, 0.007)
    img = check(backend, sp)
    assert painted(img)[:16, :16].all()
    alone = painted(check(backend, Splats(CAM32).add(3.5, 3.5, 0.3, 0.007).add(11.5, 3.5, 0.3, 0.007)))
    assert not alone.any(), "the three point splats contribute nowhere"


# ---- saturation -----------------------------------------------------------------------------------------------------------
def test_one_lane_saturates_and_63_go_on(backend):
    """three splats of opacity 0.97 and sigma 0.3 px on pixel (5, 2) (lane 21 of quadrant 0 of tile (0, 0)): T = 0.03, 9e-4, then
    2.7e-5 < 1e-4: the third is dropped there and the pixel is finished, while its neighbours (alpha 0.27) go on and take the
    splat of sigma 6 px that follows."""
    sp = Splats(CAM32).add(5, 2, 0.3, 0.97, n=3).add(7.5, 7.5, 6.0, 0.5, rgb=(1.0, 1.0, 1.0))
    img = check(backend, sp)
    only_stack = check(backend, Splats(CAM32).add(5, 2, 0.3, 0.97, n=3))
    np.testing.assert_array_equal(img[:, 2, 5], only_stack[:, 2, 5], err_msg="the finished pixel ignores the later splat")
    assert (img[:, 2, 4] > only_stack[:, 2, 4] + 0.05).all(), "its neighbour does not"
    t_left = (float(only_stack[0, 2, 5]) - sum(float(colours(i + 1)[i][0]) * 0.97 * 0.03 ** i for i in range(2))) / BG[0]
    assert abs(t_left - 9e-4) < 1e-5, "two contributions: T = 0.03^2, the third was taken back"


@pytest.mark.parametrize("first", [63, 64])
def test_every_pixel_saturates_at_one_instance(backend, first):
    """splats of sigma 400 px (alpha within 0.2 % of the opacity over the whole image): `first` - 5 of opacity 0.01, then six of
    opacity 0.8.  T before the strong ones is 0.99^58 = 0.558 (0.553); 0.558 * 0.2013^5 = 1.8e-4 >= 1e-4 and the sixth gives
    3.7e-5: all 256 pixels of every tile cross at list position `first` -- 63, the 64th and last instance of the first staged
    batch, or 64, the first of the next.  Two more splats follow and find every pixel finished."""
    sp = Splats(CAM32).add(16, 16, 400.0, 0.01, n=first - 5).add(16, 16, 400.0, 0.8, n=6).add(16, 16, 400.0, 0.5, n=2)
    lo, hi = 0.8 * np.exp(-(2 * 16.0 ** 2) / (2 * 395.0 ** 2)), 0.8
    t0 = (0.99 ** (first - 5), (1 - 0.01 * lo / 0.8) ** (first - 5))
    assert min(t0) * (1 - hi) ** 5 >= 1.2e-4 and max(t0) * (1 - lo) ** 6 < 0.8e-4, "the crossing is at the sixth strong splat everywhere"
    img = check(backend, sp)
    cut = check(backend, Splats(CAM32).add(16, 16, 400.0, 0.01, n=first - 5).add(16, 16, 400.0, 0.8, n=5))
    # the sixth strong splat is dropped and T taken back: the image of the list cut before it, but for the last bit of T * bg
    np.testing.assert_allclose(img, cut, rtol=0, atol=1e-7)


# ---- general path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", ["csc", "scs"])
def test_flagged_instances_first_middle_and_last_in_a_batch(backend, kinds):
    """a list of 66 instances over tile (0, 0): splats of sigma 4 px and opacity 0.03, and flagged ones at list positions 0, 31 and
    63 (first, middle, last slot of the first staged batch) -- c: opacity 0.99 (the alpha cap binds), s: a conic so close to
    singular that staging flags it (60 x 0.01 px, turned 45 degrees: det = 3e-4 a c).  Loop form 2 splits the runs at all
    three, form 3 only at the near-singular ones."""
    at = dict(zip((0, 31, 63), kinds))
    sp = Splats(CAM32)
    for i in range(66):
        if at.get(i) == "c":
            sp.add(4 + i % 5, 9, 1.0, 0.99)
        elif at.get(i) == "s":
            sp.add(8, 8, 60.0, 0.05, sigma2=0.01, rot=Q45)
        else:
            sp.add(7.5, 7.5, 4.0, 0.03)
    img = check(backend, sp)
    plain = check(backend, Splats(CAM32).add(7.5, 7.5, 4.0, 0.03, n=66))
    assert np.abs(img - plain)[:, :16, :16].max() > 0.2, "the flagged instances paint"


# ---- non-finite colour ----------------------------------------------------------------------------------------------------
def test_nan_colour_stays_on_its_candidate_lanes(backend):
    """a splat of sigma 0.3 px and opacity 0.5 with a NaN colour on pixel (3, 3), between splats of sigma 6 px: it is a candidate
    on the 9 pixels within 1.5 px, a part of quadrant 0 of tile (0, 0).  In the loop forms 2 and 3 those pixels are NaN and
    every other lane of the wave, which ran the same instructions under the execution mask, is finite: equal to form 0 where
    form 0 is finite (it loses the whole quadrant), and to the image of the same scene with that splat black everywhere else."""
    nan = (np.nan, np.nan, np.nan)
    sp = Splats(CAM32).add(7.5, 7.5, 6.0, 0.3).add(3, 3, 0.3, 0.5, rgb=nan).add(7.5, 7.5, 6.0, 0.4)
    clean = check(backend, Splats(CAM32).add(7.5, 7.5, 6.0, 0.3).add(3, 3, 0.3, 0.5, rgb=(0.0, 0.0, 0.0)).add(7.5, 7.5, 6.0, 0.4))
    for form in (2, 3):
        img = check(backend, sp, nan_ok=True, form=form)
        bad = np.isnan(img).any(axis=0)
        vv, uu = np.nonzero(bad)
        assert bad.sum() == 9 and ((uu - 3) ** 2 + (vv - 3) ** 2).max() == 2, "the candidates: |d|^2 <= 2"
        np.testing.assert_array_equal(img[:, ~bad], clean[:, ~bad], err_msg="the colour of a non-candidate lane is untouched")
    lost = np.isnan(check(backend, sp, nan_ok=True, form=0)).any(axis=0)
    assert lost[:8, :8].all() and lost.sum() == 64, "form 0: arithmetic masking spreads the NaN over the quadrant"


# ---- partial tiles --------------------------------------------------------------------------------------------------------
def test_partial_tiles_and_halves_of_a_list(backend):
    """40 x 24: tile column 2 is 8 px wide, tile row 1 is 8 px high -- their out-of-image lanes start finished and must stay
    inert whatever passes over them: splats of sigma 30 px over everything, point splats on the last pixel of the image and on
    the corners of the partial tiles, a stack that saturates pixel (39, 23), and splats of sigma 1.5 px that reach only the
    upper (v = 6) or only the lower (v = 22) 16 x 16 half of a 16 x 32 list."""
    sp = Splats(CAM40).add(20, 12, 30.0, 0.3, n=3)
    for u, v in ((39, 23), (32, 16), (39, 0), (0, 23), (32, 15), (31, 16)):
        sp.add(u, v, **POINT)
    sp.add(39, 23, 0.3, 0.97, n=3)
    for i in range(6):
        sp.add(4 + 6 * i, 6 if i % 2 else 22, 1.5, 0.6)
    sp.add(20, 12, 30.0, 0.5, n=2)
    img = check(backend, sp)
    assert img.shape == (3, 24, 40) and np.isfinite(img).all() and painted(img).all()
