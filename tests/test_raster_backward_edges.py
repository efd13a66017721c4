"""The rasteriser's backward pass (gs2m_rasterize_backward: k_blend_backward, the row-offset scan, k_gaussian_backward) at its
edges, on both back-ends: the frustum clamp of t.x / t.y, the scan carry past 65536 Gaussians, every SH degree and a degree below
what M holds, images below one tile and partial tiles, lists that end at the 64-instance batch boundaries, saturation and the
0.99 cap, rows that no wave writes, rotations that are not unit length, nothing to do, a dirty row arena and a backward after a
forward that overflowed its arena.

Every input is built for ONE purpose, and that purpose is asserted on the fp64 statement (tests/raster_statement.py) first, so
a case that stops reaching its branch fails instead of passing quietly.  A statement result is computed once per case
(``oracle_of``), shared between the back-ends and never modified.

Metric: per Gaussian, not per tensor.  For tensor k and Gaussian i:  n_i = max_j |g64[i,j]|,  S = max_i n_i,
e_i = max_j |g[i,j] - g64[i,j]| / max(n_i, PHI S);  the metric is max_i e_i.  PHI = 1e-3 is a floor: Gaussians under it are held
to an absolute error.  Bound: TOL_FACTOR (4, test_raster_backward) x the SAME metric of the SAME statement evaluated in fp32 on
the CPU -- independent of the code under test.  The per-tensor check of test_raster_backward is applied too.  Where the
kernels exceed 4 x the one row-by-row fp32 evaluation, ``judge`` takes, FOR THAT ENTRY ONLY, the worst of ORDERS more fp32
evaluations of the statement as the yardstick (statement only), prints the use and keeps the factor.  Loss and
weights are those of test_raster_backward: seeded w, zeroed on pixels with a decision within 1e-4 of its threshold
(oracle.render_flip_bounds), at most 1 % of the pixels.  Measured figures: profiles/raster_backward_edges.txt (``-s`` prints
them).
"""
import functools

import numpy as np
import pytest
import torch

import oracle
import raster_statement as rs
from gs2mesh_amd import synthetic
from gs2mesh_amd.rasterizer import Rasterizer
from gs2mesh_amd.sh_utils import RGB2SH
from test_raster_backward import TENSORS, TOL_FACTOR, errors

PHI = 1e-3
ORDERS = 8           # pixel orders of the fp32 statement behind the yardstick of an ill-conditioned sum
E32_CEILING = 1e-3   # no fp32 evaluation of the statement may be further from the fp64 one: a broken yardstick fails loudly
BG = np.array([0.1, 0.2, 0.3], np.float32)


# ---- the metric ---------------------------------------------------------------------------------------------------------
def per_gaussian(g, g64):
    """-> {tensor: (e_i[P], n_i[P], S)}; None where the oracle's tensor is identically zero"""
    out = {}
    for k in TENSORS:
        if g64.get(k) is None:
            continue
        ref = np.asarray(g64[k], np.float64)
        ref = ref.reshape(ref.shape[0], -1)
        d = np.abs(np.asarray(g[k], np.float64).reshape(ref.shape) - ref).max(axis=1, initial=0.0)
        n = np.abs(ref).max(axis=1, initial=0.0)
        S = n.max(initial=0.0)
        out[k] = None if S == 0 else (d / np.maximum(n, PHI * S), n, S)
    return out


def judge(name, g, only=None, label=None):
    """The bound is TOL_FACTOR x the fp32 statement, per tensor (max and relative L2, the check of test_raster_backward) and
    per Gaussian (max_i e_i).  Where the kernels exceed it, the statement alone decides whether THAT entry is ill-conditioned,
    and only that entry gets another yardstick -- a (tensor, metric) of the per-tensor check, a (tensor, Gaussian) of the
    per-Gaussian one; every other entry of the case keeps the row-by-row bound:
      1. the worst of the row-by-row fp32 statement and ORDERS more fp32 evaluations, each summing the gradients over the pixels
         in another seeded order (for a Gaussian: the worst error of THAT Gaussian over the orders, or the tensor's row-by-row
         figure if that is larger);
      2. if that is not enough, the same with the transmittance built from the back of the list, T_final divided by the
         (1 - alpha) behind, as the reference's backward builds it (backward.cu:503).  This is another fp32 evaluation of the
         same function, not an order of the contributors: it is the yardstick of the front of a long list, which carries the
         rounding of the whole division chain in any backward that rebuilds T that way.
    The factor stays TOL_FACTOR, no yardstick may exceed E32_CEILING, and nothing of it depends on the code under test.  Every
    use is printed as a WIDER line (profiles/raster_backward_edges.txt, section 4)."""
    label = label or name
    g64, e32, pg32, _ = oracle_of(name)
    bad = []
    # ---- per tensor
    for k, v in errors(g, g64).items():
        print(f"[{label}] {k:8s} e32 = {e32[k]}  hip = {v}")
        if v is None:
            assert not np.asarray(g[k]).any(), f"{k}: the oracle's gradient is identically zero"
            continue
        for m, metric in enumerate(("max", "l2")):
            if v[m] <= TOL_FACTOR * e32[k][m]:
                continue
            for stage, back in (("pixel orders", False), ("T from the back", True)):
                y = max([e32[k][m]] + [o[0][k][m] for o in orders(name, back)])
                assert y <= E32_CEILING, f"{label}: the yardstick of {k} {metric} is {y:.2e}: the fp32 statement is broken"
                ok = v[m] <= TOL_FACTOR * y
                if ok or back:
                    print(f"[{label}] WIDER per-tensor {k} {metric}: krn = {v[m]:.3e}  row-by-row e32 = {e32[k][m]:.3e}  "
                          f"{stage} e32 = {y:.3e}  ratio = {v[m] / y:.2f}")
                if ok:
                    break
            else:
                bad.append((k, metric, v[m], e32[k][m], y))
    # ---- per Gaussian
    for k, v in per_gaussian(g, g64).items():
        if v is None:
            assert not np.asarray(g[k]).any(), f"{k}: the oracle's gradient is identically zero"
            print(f"[{label}] per-Gaussian {k:8s} zero")
            continue
        e = v[0] if only is None else np.where(only, v[0], 0.0)
        y0 = float(pg32[k][0].max())
        i = int(np.argmax(e))
        print(f"[{label}] per-Gaussian {k:8s} e32 = {y0:.3e}  krn = {e[i]:.3e}  ratio = {e[i] / y0:.2f}  (worst id {i})")
        for i in np.nonzero(e > TOL_FACTOR * y0)[0]:
            for stage, back in (("pixel orders", False), ("T from the back", True)):
                y = max([y0] + [float(o[1][k][0][i]) for o in orders(name, back)])
                assert y <= E32_CEILING, f"{label}: the yardstick of {k}[{i}] is {y:.2e}: the fp32 statement is broken"
                ok = e[i] <= TOL_FACTOR * y
                if ok or back:
                    print(f"[{label}] WIDER per-Gaussian {k} id {i}: krn = {e[i]:.3e}  row-by-row e32 = {y0:.3e}  "
                          f"{stage} e32 of this Gaussian = {y:.3e}  ratio = {e[i] / y:.2f}  n_i / S = {v[1][i] / v[2]:.2e}")
                if ok:
                    break
            else:
                bad.append((k, int(i), e[i], y0, y))
    assert not bad, f"{label}: beyond {TOL_FACTOR} x the fp32 statement's error, row by row and in every other evaluation: {bad}"


# ---- building blocks of the designed scenes ----------------------------------------------------------------------------
def camera(W, H, f):
    """identity pose: world = view space, +z forward; the centre of pixel (u, v) at depth z is place(u, v, z)"""
    return synthetic.stereo_cameras(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), W, H, f, f, 0.245)[0]


def place(u, v, z, W, H, f):
    u, v, z = (np.asarray(a, np.float64) for a in np.broadcast_arrays(u, v, z))
    return np.stack([(u - 0.5 * W + 0.5) * z / f, (v - 0.5 * H + 0.5) * z / f, z], axis=1).astype(np.float32)


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def scales_px(rng, sigma_px, z, f, aniso=0.3):
    """world scales [n,3] whose projected sigma is sigma_px (x a per-axis factor in 1 +- aniso)"""
    sigma_px, z = np.broadcast_arrays(np.asarray(sigma_px, np.float64), np.asarray(z, np.float64))
    return (sigma_px[:, None] * z[:, None] / f * rng.uniform(1 - aniso, 1 + aniso, (z.size, 3))).astype(np.float32)


def random_shs(rng, n, M=16):
    shs = rng.normal(0.0, 0.05, (n, M, 3))
    shs[:, 0] = RGB2SH(rng.uniform(0.0, 1.0, (n, 3)))
    return shs.astype(np.float32)


def finish(name, xyz, s, q, o, shs, W, H, f, deg=3, seed=77):
    """-> the case dict of test_raster_backward.case: inputs, camera, the seeded weights with the threshold pixels zeroed"""
    cam = camera(W, H, f)
    xyz, s, q, shs = (np.ascontiguousarray(a, np.float32) for a in (xyz, s, q, shs))
    o = np.ascontiguousarray(o, np.float32).reshape(-1)
    arrays = dict(means3D=xyz, opacities=o, shs=shs, colors_precomp=None, scales=s, rotations=q, cov3D_precomp=None)
    geom = oracle.preprocess(xyz, s, q, o, shs, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, W, H,
                             cam.tanfovx, cam.tanfovy, sh_degree=deg)
    pl, ranges = oracle.bin_instances(geom, W, H)
    fb = oracle.render_flip_bounds(W, H, ranges, pl, geom["means2D"], geom["conic_opacity"], 1.0, rel_eps=1e-4)
    near = (fb["n_alpha"].astype(np.int64) + fb["n_T"] + fb["n_power"]) > 0
    w = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, H, W)).astype(np.float32)
    w[:, near] = 0.0
    for a in (xyz, s, q, o, shs, w):
        a.setflags(write=False)
    return dict(name=name, arrays=arrays, cam=cam, W=W, H=H, bg=BG, deg=deg, mod=1.0, w=w, zeroed=float(near.mean()), geom=geom)


# ---- case 1: the frustum clamp ------------------------------------------------------------------------------------------
def clamp_case():
    """64 x 48.  The forward clamps t.x / t.z to +-1.3 tan(fov): a centre more than 0.3 W / 2 = 9.6 px beyond the left / right
    edge (0.3 H / 2 = 7.2 px beyond top / bottom) is clamped.  6 Gaussians clamped in x only, 6 in y only, 8 in both, both signs
    each, 12..18 px outside with sigma 11..14 px (3 sigma reaches 15 px and more into the image) and opacity 0.6..0.9; 20
    unclamped neighbours inside the image and up to 5 px outside it."""
    W, H, f = 64, 48, 60.0
    rng = np.random.default_rng(101)
    out = lambda n: rng.uniform(12.0, 18.0, n)
    ux = np.concatenate([-out(3), W - 1 + out(3)])                    # x only: v inside
    vx = rng.uniform(6, H - 7, 6)
    uy = rng.uniform(8, W - 9, 6)                                     # y only: u inside
    vy = np.concatenate([-out(3), H - 1 + out(3)])
    ub = np.concatenate([-out(4), W - 1 + out(4)])                    # both: the four corners, two each
    vb = np.concatenate([-out(2), H - 1 + out(2), -out(2), H - 1 + out(2)])
    un = rng.uniform(-5, W + 4, 20)
    vn = rng.uniform(-5, H + 4, 20)
    u, v = np.concatenate([ux, uy, ub, un]), np.concatenate([vx, vy, vb, vn])
    n = u.size
    z = rng.uniform(2.0, 4.0, n)
    sigma = np.concatenate([rng.uniform(11.0, 14.0, 20), rng.uniform(3.0, 9.0, 20)])
    o = np.concatenate([rng.uniform(0.6, 0.9, 20), rng.uniform(0.2, 0.9, 20)])
    c = finish("clamp", place(u, v, z, W, H, f), scales_px(rng, sigma, z, f), unit_quats(rng, n), o, random_shs(rng, n), W, H, f)
    c["classes"] = dict(x_only=np.arange(0, 6), y_only=np.arange(6, 12), both=np.arange(12, 20), none=np.arange(20, 40))
    return c


# ---- case 2: the carry of the row-offset scan ---------------------------------------------------------------------------
SCAN_P = 2 * 65536 + 700
SCAN_BLOCKS = (0, 255, 256, 257, 511, 512, 514)      # 256 Gaussians per block; 514 is the last, partial one (188 ids)


@functools.lru_cache(maxsize=None)
def scan_scenes(seed=202):
    """-> (big: SCAN_P Gaussians, all behind the camera but 43 in each block of SCAN_BLOCKS; compact: the visible ones in the
    same order; visible ids).  k_bw_scan_blocks scans the 515 block sums in rounds of 256: blocks 256.. need the carry of round 0,
    blocks 512.. that of rounds 0 and 1.  M = 4, D = 1 keeps the big scene small."""
    W, H, f = 64, 48, 60.0
    rng = np.random.default_rng(seed)
    ids = np.concatenate([256 * b + np.sort(rng.choice(188, 43, replace=False)) for b in SCAN_BLOCKS])
    n = ids.size
    z = rng.uniform(2.0, 4.0, n)
    xyz_v = place(rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), z, W, H, f)
    s_v, q_v = scales_px(rng, rng.uniform(2.0, 5.0, n), z, f), unit_quats(rng, n)
    o_v, sh_v = rng.uniform(0.05, 0.5, n).astype(np.float32), random_shs(rng, n, 4)
    xyz = np.zeros((SCAN_P, 3), np.float32)
    xyz[:, :2] = rng.uniform(-1, 1, (SCAN_P, 2))
    xyz[:, 2] = rng.uniform(-4.0, -1.0, SCAN_P)       # behind the camera
    s = np.full((SCAN_P, 3), 0.1, np.float32)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (SCAN_P, 1))
    o = np.full(SCAN_P, 0.5, np.float32)
    shs = np.zeros((SCAN_P, 4, 3), np.float32)
    xyz[ids], s[ids], q[ids], o[ids], shs[ids] = xyz_v, s_v, q_v, o_v, sh_v
    big = finish("scan/big", xyz, s, q, o, shs, W, H, f, deg=1)
    compact = finish("scan", xyz_v, s_v, q_v, o_v, sh_v, W, H, f, deg=1)
    return big, compact, ids


# ---- case 3: SH degrees -------------------------------------------------------------------------------------------------
SH_VARIANTS = [(0, 16), (1, 16), (2, 16), (3, 16), (1, 4), (2, 9)]


def sh_case(D, M, scaled_rot=False):
    """300 Gaussians at 96 x 80, the same for every (D, M) but for the trailing coefficients M cuts off.  Gaussians 0..9 have
    a DC term that clamps every channel, 10..19 one that clamps the red channel only.  ``scaled_rot``: the quaternions are
    multiplied by factors in 0.7..1.4 (20..39: evenly spaced over that range) and NOT normalised (operator and statement both
    take q as given)."""
    W, H, f = 96, 80, 90.0
    rng = np.random.default_rng(303)
    n = 300
    z = rng.uniform(2.0, 5.0, n)
    xyz = place(rng.uniform(-4, W + 3, n), rng.uniform(-4, H + 3, n), z, W, H, f)
    s, q = scales_px(rng, rng.uniform(1.5, 7.0, n), z, f), unit_quats(rng, n)
    o = rng.uniform(0.05, 0.95, n)
    shs = random_shs(rng, n)
    shs[:, 1:] *= 4.0                                  # the view-dependent part matters
    shs[:10, 0] = -8.0
    shs[10:20, 0, 0] = -8.0
    # the Gaussians the case is about, 0..39, are in front, inside the image, mid-sized and fairly opaque
    z[:40] = 1.5 + 0.01 * np.arange(40)
    xyz[:40] = place(rng.uniform(8, W - 9, 40), rng.uniform(8, H - 9, 40), z[:40], W, H, f)
    s[:40] = scales_px(rng, rng.uniform(3.0, 5.0, 40), z[:40], f)
    o[:40] = rng.uniform(0.4, 0.8, 40)
    if scaled_rot:
        factor = rng.uniform(0.7, 1.4, (n, 1))
        factor[20:40, 0] = np.linspace(0.7, 1.4, 20)
        q = q * factor.astype(np.float32)
    return finish(f"sh{D}_{M}" + ("_rot" if scaled_rot else ""), xyz, s, q, o, shs[:, :M], W, H, f, deg=D)


# ---- case 4: image sizes ------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 5), (16, 16), (17, 16), (16, 17), (33, 47)]


def size_case(W, H, seed=410):
    """60 Gaussians: 0 covers every tile, 1..4 straddle the left / right / top / bottom edge, 5..8 lie entirely outside (their
    rect is empty: radius 0), the rest are scattered over the image (in the smallest images they pile up and the pixels saturate)."""
    f = 0.9 * max(W, H) + 4.0
    rng = np.random.default_rng(seed + 100 * W + H)
    n = 60
    u, v = rng.uniform(-1, W, n), rng.uniform(-1, H, n)
    sigma = rng.uniform(0.8, 1.0 + 0.15 * max(W, H), n)
    o = rng.uniform(0.1, 0.9, n)
    u[0], v[0], sigma[0], o[0] = 0.5 * W, 0.5 * H, 2.0 * max(W, H) + 8, 0.3
    edge = 2.0 + 0.05 * max(W, H)
    u[1:5] = [-1.0, W, 0.5 * W, 0.5 * W]
    v[1:5] = [0.5 * H, 0.5 * H, -1.0, H]
    sigma[1:5] = edge
    u[5:9] = [-40.0 - W, 2 * W + 40.0, 0.5 * W, 0.5 * W]
    v[5:9] = [0.5 * H, 0.5 * H, -40.0 - H, 2 * H + 40.0]
    sigma[5:9] = 1.0
    z = rng.uniform(2.0, 4.0, n)
    z[:5] = 1.5 + 0.01 * np.arange(5)                  # in front: they contribute whatever piles up behind them
    return finish(f"size{W}x{H}", place(u, v, z, W, H, f), scales_px(rng, sigma, z, f, aniso=0.2), unit_quats(rng, n), o,
                  random_shs(rng, n), W, H, f)


# ---- case 5: list ends --------------------------------------------------------------------------------------------------
LIST_N = [1, 63, 64, 65, 128, 129]
TAIL = 70


def list_case(n, tail=False):
    """one 16 x 16 tile, exactly n Gaussians that all cover it (sigma 6..12 px, centres inside), depth increasing with the id,
    opacity 0.02..0.05: (1 - 0.05)^129 = 1.3e-3, nothing saturates.  The last of the n is wide and at opacity 0.05, so it
    contributes and max n_contrib = n.  ``tail``: TAIL more Gaussians behind them with opacity 0.003 < 1 / 255: in the list
    (radius > 0), never a contributor, so the list is longer than the wave's largest n_contrib and their rows are never written."""
    W = H = 16
    f = 20.0
    rng = np.random.default_rng(505 + n)
    m = n + (TAIL if tail else 0)
    z = 2.0 + 0.01 * np.arange(m)
    sigma = rng.uniform(6.0, 12.0, m)
    o = rng.uniform(0.02, 0.05, m)
    sigma[n - 1], o[n - 1] = 12.0, 0.05
    o[n:] = 0.003
    xyz = place(rng.uniform(3, 12, m), rng.uniform(3, 12, m), z, W, H, f)
    return finish(f"list{n}" + ("_tail" if tail else ""), xyz, scales_px(rng, sigma, z, f, aniso=0.15), unit_quats(rng, m), o,
                  random_shs(rng, m), W, H, f)


# ---- case 6: saturation and the cap -------------------------------------------------------------------------------------
SAT_FRONT, SAT_FAINT, SAT_SLABS, SAT_BEHIND = 8, 280, 30, 10


def sat_case(seed=606):
    """32 x 16, two tiles, every list longer than 128.  Front to back:
      * 8 strong Gaussians (sigma 2.5..3.2 px, opacity 0.9 or 1.0, ON pixel centres) clustered in x 3..5, y 6..9 (an integer
        centre plus an integer radius may not reach 17: that is exactly the edge of the next tile, decided by the last bit): the pixels
        there saturate within the first 64 instances, in few large steps (many small ones would linger at the 1e-4 threshold);
      * 280 faint ones (sigma 1..1.3 px, opacity 0.006..0.009: over 1 / 255 within a pixel or two of the centre) everywhere,
        each in the list of its own tile mostly: they move the list position, not T;
      * one cover at opacity 0.3, so that no pixel meets two capped hits from T = 1 (0.01^2 sits ON the 1e-4 threshold);
      * 30 slabs (sigma 80..120 px, ON pixel centres), two of three at opacity 1.0 -- min(0.99, o G) binds within 0.14 sigma of the
        centre -- the others at 0.9..0.97: every remaining pixel saturates here, at list positions beyond 128;
      * 10 more slabs behind every pixel's last contributor: their gradients are exactly zero."""
    W, H, f = 32, 16, 30.0
    rng = np.random.default_rng(seed)
    k = [SAT_FRONT, SAT_FAINT, 1, SAT_SLABS, SAT_BEHIND]
    n = sum(k)
    u = np.concatenate([rng.integers(3, 6, k[0]), rng.uniform(0, W - 1, k[1]), [15.5], rng.integers(0, W, k[3] + k[4])]).astype(float)
    v = np.concatenate([rng.integers(6, 10, k[0]), rng.uniform(0, H - 1, k[1]), [7.5], rng.integers(0, H, k[3] + k[4])]).astype(float)
    sigma = np.concatenate([rng.uniform(2.5, 3.2, k[0]), rng.uniform(1.0, 1.3, k[1]), [60.0], rng.uniform(80, 120, k[3] + k[4])])
    slab_o = np.where(np.arange(k[3] + k[4]) % 3 == 2, rng.uniform(0.9, 0.97, k[3] + k[4]), 1.0)
    o = np.concatenate([np.where(np.arange(k[0]) % 2 == 0, 1.0, 0.9), rng.uniform(0.006, 0.009, k[1]), [0.3], slab_o])
    z = 2.0 + 0.01 * np.arange(n)
    c = finish("sat", place(u, v, z, W, H, f), scales_px(rng, sigma, z, f, aniso=0.1), unit_quats(rng, n), o, random_shs(rng, n),
               W, H, f)
    c["behind"] = np.arange(n - SAT_BEHIND, n)
    return c


# ---- case 7: nothing to do ----------------------------------------------------------------------------------------------
def culled_case():
    """50 Gaussians, none rendered: 25 behind the camera, 25 in front of it and far outside the image (empty rect)"""
    W, H, f = 33, 47, 40.0
    rng = np.random.default_rng(707)
    n = 50
    z = np.concatenate([rng.uniform(-4.0, 0.1, 25), rng.uniform(2.0, 4.0, 25)])
    u = np.concatenate([rng.uniform(0, W, 25), 10.0 * W + rng.uniform(0, W, 25)])
    xyz = place(u, rng.uniform(0, H, n), np.where(z == 0, 1.0, z), W, H, f)
    return finish("culled", xyz, scales_px(rng, 2.0, np.abs(z) + 1.0, f), unit_quats(rng, n), rng.uniform(0.1, 0.9, n),
                  random_shs(rng, n), W, H, f)


def single_case():
    W, H, f = 33, 47, 40.0
    rng = np.random.default_rng(708)
    return finish("single", place([14.3], [20.6], [3.0], W, H, f), scales_px(rng, [5.0], [3.0], f), unit_quats(rng, 1), [0.7],
                  random_shs(rng, 1), W, H, f)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "clamp":
        return clamp_case()
    if name == "scan":
        return scan_scenes()[1]
    if name.startswith("sh"):
        D, M = name[2:].split("_")[:2]
        return sh_case(int(D), int(M), name.endswith("_rot"))
    if name.startswith("size"):
        W, H = name[4:].split("x")
        return size_case(int(W), int(H))
    if name.startswith("list"):
        return list_case(int(name[4:].split("_")[0]), name.endswith("_tail"))
    return dict(sat=sat_case, culled=culled_case, single=single_case)[name]()


def statement_grads(c, dtype, **render_kw):
    """test_raster_backward.statement_grads with the keyword switches of rs.render"""
    p = rs.leaves(c["arrays"], dtype)
    img, aux = rs.render(p, c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"], **render_kw)
    (img * torch.tensor(c["w"], dtype=dtype)).sum().backward()
    z = lambda t, like: np.zeros(like, np.float64) if t is None or t.grad is None else t.grad.detach().numpy().astype(np.float64)
    P = c["arrays"]["means3D"].shape[0]
    ca, cb, cc = aux["t_conic"]
    conic = np.stack([z(ca, P), 0.5 * z(cb, P), np.zeros(P), z(cc, P)], axis=1)   # dL_dconic.y is half the derivative
    g = dict(mean2D=z(p["means2D"], (P, 3)), conic=conic, opacity=z(p["opacities"], P), color=z(aux["t_rgb"], (P, 3)),
             mean3D=z(p["means3D"], (P, 3)), cov3D=z(aux["t_cov3"], (P, 6)), sh=z(p["shs"], tuple(p["shs"].shape)),
             scale=z(p["scales"], (P, 3)), rot=z(p["rotations"], (P, 4)))
    return g, img.detach().numpy(), aux


def assert_same_scene(name, what, aux, aux64, keep):
    """an fp32 evaluation differentiates the SAME scene as the fp64 one: equal radii, rects and lists, and on every pixel that
    carries weight the same last contributor and the same saturating instance"""
    for k in ("radii", "rect", "tile_len"):
        np.testing.assert_array_equal(aux[k], aux64[k], err_msg=f"{name}: {k} of the {what} statement")
    for k in ("n_contrib", "sat_at"):
        np.testing.assert_array_equal(aux[k][keep], aux64[k][keep], err_msg=f"{name}: {k} of the {what} statement")


@functools.lru_cache(maxsize=None)
def orders(name, back):
    """-> [(per-tensor errors, per-Gaussian errors)] of ORDERS more fp32 evaluations of the statement, a seeded pixel order
    each; ``back``: with the transmittance multiplied up from the back of the list (the order of the reference's backward)"""
    c = case(name)
    g64, _, _, aux64 = oracle_of(name)
    out = []
    for seed in range(1, ORDERS + 1):
        g32, _, aux = statement_grads(c, torch.float32, pixel_order_seed=seed, transmittance_from_back=back)
        assert_same_scene(name, f"fp32 order {seed}", aux, aux64, c["w"][0] != 0)
        out.append((errors(g32, g64), per_gaussian(g32, g64)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """-> (g64, e32 = per-tensor errors of the fp32 statement, pg32 = its per-Gaussian errors, aux of the fp64 run).  Asserts
    that what is differentiated IS the reference's function (image against oracle.rasterize_forward, radii and rects against
    oracle.preprocess), that the fp32 statement differentiates the same scene and stays under E32_CEILING, and that at most
    1 % of the pixels lost their weight."""
    c = case(name)
    assert c["zeroed"] <= 0.01, f"{name}: {c['zeroed']:.2%} of the pixels sit on a threshold"
    g64, img64, aux = statement_grads(c, torch.float64)
    a = c["arrays"]
    cam = c["cam"]
    ref_img, ref_radii, _ = oracle.rasterize_forward(
        a["means3D"], a["opacities"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center, c["W"], c["H"],
        cam.tanfovx, cam.tanfovy, c["bg"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"], sh_degree=c["deg"])
    keep = c["w"][0] != 0
    assert np.abs(img64 - ref_img)[:, keep].max(initial=0.0) <= 2e-4
    np.testing.assert_array_equal(aux["radii"], ref_radii)
    vis = ref_radii > 0
    np.testing.assert_array_equal(aux["rect"][vis], c["geom"]["rect"][vis])
    g32, _, aux32 = statement_grads(c, torch.float32)
    assert_same_scene(name, "row-by-row fp32", aux32, aux, keep)
    e32, pg32 = errors(g32, g64), per_gaussian(g32, g64)
    worst = max([max(v) for v in e32.values() if v is not None] + [float(v[0].max()) for v in pg32.values() if v is not None])
    assert worst <= E32_CEILING, f"{name}: the fp32 statement is {worst:.2e} from the fp64 one: a broken yardstick"
    print(f"[{name}] statement: P = {vis.size}, visible = {int(vis.sum())}, zeroed pixels = {c['zeroed']:.2%}, saturated pixels = "
          f"{aux['saturated'].mean():.1%}, cap binds in {aux['capped']} of {aux['contributing']} contributing evaluations, "
          f"longest list = {int(aux['tile_len'].max())}, max n_contrib = {int(aux['n_contrib'].max())}, worst e32 = {worst:.1e}")
    return g64, e32, pg32, aux


def assert_above_floor(name, ids, tensors):
    """every Gaussian the case is about is judged by its RELATIVE error: n_i >= PHI S in the tensors concerned"""
    ids = np.asarray(ids)
    pg = per_gaussian(oracle_of(name)[0], oracle_of(name)[0])
    for k in tensors:
        _, n, S = pg[k]
        assert (n[ids] >= PHI * S).all(), f"{name}: {k} of Gaussians {ids[n[ids] < PHI * S]} is under the floor"


# ---- running the library --------------------------------------------------------------------------------------------------
def run(be, c, r=None, w=None, nan_fill=True, forward=True):
    """forward + backward of case c on back-end be (on handle r, or a fresh one), every fp32 output buffer NaN-filled first
    -> (gradients as numpy, radii, handle)"""
    import gs2mesh_amd.rasterizer as rz
    a, cam = c["arrays"], c["cam"]
    d = lambda v: None if v is None else be.dev(np.array(v))   # a writable copy: the cases themselves are read-only
    r = r or Rasterizer(0, lib=be.lib)
    dev = {k: d(v) for k, v in a.items() if k not in ("means3D", "opacities")}
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"],
              cam.tanfovx, cam.tanfovy)
    xyz = d(a["means3D"])
    real_empty = rz._empty

    def nan_empty(like, shape, np_dtype):
        t = real_empty(like, shape, np_dtype)
        if np_dtype == np.float32:
            t[...] = float("nan")
        return t

    rz._empty = nan_empty if nan_fill else real_empty
    try:
        radii = None
        if forward:
            _, radii = r.forward(xyz, d(a["opacities"]), *common, sh_degree=c["deg"], **dev)
        g = r.backward(d(c["w"] if w is None else w), xyz, *common, sh_degree=c["deg"], want_conic=True, **dev)
        be.sync()
    finally:
        rz._empty = real_empty
    g = {k: (None if v is None else be.host(v).copy()) for k, v in g.items()}
    P = a["means3D"].shape[0]
    for k, v in g.items():
        if v is not None:
            assert v.shape[0] == P and np.isfinite(v).all(), f"{k}: not fully written"
    return g, (None if radii is None else be.host(radii)), r


def assert_zero(g, ids, what):
    for k, v in g.items():
        if v is not None:
            assert not v[ids].any(), f"{k}: non-zero gradient for {what}"


def assert_bitwise(g1, g2):
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None)
        if g1[k] is not None:
            assert g1[k].tobytes() == g2[k].tobytes(), k


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def test_frustum_clamp_passes_no_gradient_to_tx_ty(backend):
    c = case("clamp")
    g64, e32, pg32, aux = oracle_of("clamp")
    cls = c["classes"]
    cx, cy = aux["clamped_x"], aux["clamped_y"]
    assert (aux["radii"][:20] > 0).all(), "every clamped Gaussian is rendered"
    assert (cx[cls["x_only"]] & ~cy[cls["x_only"]]).all() and (~cx[cls["y_only"]] & cy[cls["y_only"]]).all()
    assert (cx[cls["both"]] & cy[cls["both"]]).all() and not (cx[cls["none"]] | cy[cls["none"]]).any()
    tv = c["arrays"]["means3D"]
    for ids, axes in ((cls["x_only"], (0,)), (cls["y_only"], (1,)), (cls["both"], (0, 1))):
        for ax in axes:
            assert (tv[ids, ax] > 0).sum() >= 2 and (tv[ids, ax] < 0).sum() >= 2, "both signs"
    assert len(cls["x_only"]) >= 4 and len(cls["y_only"]) >= 4 and len(cls["both"]) >= 4
    clamped = np.arange(20)
    assert_above_floor("clamp", clamped, ("mean3D", "mean2D", "opacity", "cov3D"))
    # each clamped Gaussian contributes to image pixels: its colour gradient is not zero
    assert (np.abs(g64["color"][clamped]).max(axis=1) > 0).all()
    # the case tells the contract from the plain derivative of the clamp: > 100 x the bound for EVERY clamped Gaussian
    p = rs.leaves(c["arrays"], torch.float64)
    img, _ = rs.render(p, c["cam"], c["W"], c["H"], c["bg"], c["deg"], c["mod"], clamp_passes_gradient=True)
    (img * torch.tensor(c["w"], dtype=torch.float64)).sum().backward()
    wrong = p["means3D"].grad.numpy()
    _, n, S = per_gaussian(g64, g64)["mean3D"]
    e_wrong = np.abs(wrong - g64["mean3D"]).max(axis=1) / np.maximum(n, PHI * S)
    bound = TOL_FACTOR * float(pg32["mean3D"][0].max())
    print(f"[clamp] classes x_only/y_only/both/none = {[len(v) for v in cls.values()]}, wrong derivative / bound: min over the "
          f"clamped = {e_wrong[clamped].min() / bound:.0f}, max over the unclamped = {e_wrong[cls['none']].max() / bound:.2g}")
    assert (e_wrong[clamped] > 100 * bound).all()
    assert (e_wrong[cls["none"]] == 0).all()
    g, radii, _ = run(backend, c)
    np.testing.assert_array_equal(radii, aux["radii"])
    judge("clamp", g)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_scan_carry_beyond_65536_gaussians(backend):
    big, compact, ids = scan_scenes()
    g64, e32, pg32, aux = oracle_of("scan")
    area = (aux["rect"][:, 2].astype(np.int64) - aux["rect"][:, 0]) * (aux["rect"][:, 3].astype(np.int64) - aux["rect"][:, 1])
    assert big["arrays"]["means3D"].shape[0] == SCAN_P == 2 * 65536 + 700
    assert sorted(set(ids // 256)) == list(SCAN_BLOCKS) and SCAN_P - 256 * 514 < 256
    for lo in (65536, 131072):
        assert ((ids >= lo) & (aux["radii"] > 0) & (area > 1)).any(), f"no visible multi-tile Gaussian at id >= {lo}"
    print(f"[scan] visible {int((aux['radii'] > 0).sum())} of {SCAN_P}, rows = {int(area.sum())}, multi-tile rects at ids >= "
          f"65536: {int(((ids >= 65536) & (area > 1)).sum())}, >= 131072: {int(((ids >= 131072) & (area > 1)).sum())}")
    g_big, radii_big, r_big = run(backend, big)
    g_cmp, radii_cmp, r_cmp = run(backend, compact)
    visible = np.zeros(SCAN_P, bool)
    visible[ids] = True
    np.testing.assert_array_equal(radii_big[ids], aux["radii"])
    assert not radii_big[~visible].any()
    assert r_big.backward_rows()[0] == r_cmp.backward_rows()[0] == int(area.sum())
    # the sorted lists are the same up to relabelling and rows are summed in slot order: the same bits
    assert_bitwise({k: (None if v is None else v[ids]) for k, v in g_big.items()}, g_cmp)
    assert_zero(g_big, ~visible, "a Gaussian behind the camera")
    judge("scan", g_cmp)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _sh_test(backend, name, D, M):
    g64, e32, pg32, aux = oracle_of(name)
    vis = aux["radii"] > 0
    cl = aux["rgb_clamped"]
    assert (vis & cl.all(axis=1)).any(), "a visible Gaussian with every channel clamped"
    assert (vis & cl.any(axis=1) & ~cl.all(axis=1)).any(), "a visible Gaussian with a mixed clamp"
    ncoef = (D + 1) ** 2
    assert g64["sh"].shape[1] == M and not g64["sh"][:, ncoef:].any() and np.abs(g64["sh"][:, ncoef - 1]).max() > 0
    assert cl[:10].all() and cl[10:20, 0].all() and not cl[10:20].all(axis=1).any() and vis[:40].all()
    assert_above_floor(name, np.arange(0, 10), ("color", "opacity", "mean2D"))      # sh is exactly zero: every channel clamped
    assert_above_floor(name, np.arange(10, 20), ("sh", "color", "opacity", "mean3D"))
    g, _, _ = run(backend, case(name))
    assert g["sh"].shape == g64["sh"].shape
    assert not g["sh"][:, ncoef:].any(), "coefficients above the active degree get exactly zero"
    assert not g["sh"][cl[:, None, :].repeat(M, axis=1)].any(), "clamped channels pass no gradient"
    judge(name, g)


@pytest.mark.parametrize("D,M", SH_VARIANTS)
def test_sh_degree_and_coefficient_count(backend, D, M):
    _sh_test(backend, f"sh{D}_{M}", D, M)


@pytest.mark.parametrize("D", [0, 1])
def test_coefficients_above_the_active_degree_are_not_read(backend, D):
    """training runs D = 0 with M = 16 and raises D later: whatever the coefficients above (D + 1)^2 hold, NaN included, is
    neither read nor written to by the backward -- 0 x NaN would reach dL_dmean3D through the view direction otherwise"""
    c = case(f"sh{D}_16")
    shs = np.array(c["arrays"]["shs"])
    shs[:, (D + 1) ** 2:] = np.nan
    g_nan, _, _ = run(backend, dict(c, arrays=dict(c["arrays"], shs=shs)))     # run() asserts that every output is finite
    g, _, _ = run(backend, c)
    assert not g_nan["sh"][:, (D + 1) ** 2:].any()
    assert_bitwise(g_nan, g)


def test_rotations_that_are_not_unit_length(backend):
    c = case("sh3_16_rot")
    norm = np.linalg.norm(c["arrays"]["rotations"], axis=1)
    assert norm.min() < 0.75 and norm.max() > 1.3
    g64 = oracle_of("sh3_16_rot")[0]
    # the gradient has a radial part only because q is NOT normalised inside the operator
    radial = np.abs((g64["rot"] * c["arrays"]["rotations"]).sum(axis=1))
    assert radial.max() > 0.1 * np.abs(g64["rot"]).max()
    assert norm[20] < 0.71 and norm[39] > 1.39
    assert_above_floor("sh3_16_rot", np.arange(20, 40), ("rot", "scale", "cov3D"))
    _sh_test(backend, "sh3_16_rot", 3, 16)


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_image_sizes_below_and_across_a_tile(backend, W, H):
    name = f"size{W}x{H}"
    c = case(name)
    g64, e32, pg32, aux = oracle_of(name)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    radii, rect = aux["radii"], aux["rect"].astype(np.int64)
    m2 = c["geom"]["means2D"]
    assert radii[0] > 0 and tuple(rect[0]) == (0, 0, gx, gy), "Gaussian 0 covers every tile"
    assert (radii[1:5] > 0).all()
    assert m2[1, 0] - radii[1] < 0 and m2[2, 0] + radii[2] > W - 1 and m2[3, 1] - radii[3] < 0 and m2[4, 1] + radii[4] > H - 1
    assert_above_floor(name, [0], ("opacity", "color"))
    assert_above_floor(name, np.arange(1, 5), ("opacity", "color", "mean2D", "mean3D"))   # the Gaussians the image clips contribute
    assert not radii[5:9].any() and (c["arrays"]["means3D"][5:9, 2] > 0.2).all(), "in front of the camera, outside the image"
    g, hip_radii, r = run(backend, c)
    np.testing.assert_array_equal(hip_radii, radii)
    assert r.backward_rows()[0] == int(((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).sum())
    assert_zero(g, radii == 0, "a culled Gaussian")
    judge(name, g)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("n", LIST_N)
def test_lists_that_end_at_batch_boundaries(backend, n, tail):
    name = f"list{n}" + ("_tail" if tail else "")
    c = case(name)
    g64, e32, pg32, aux = oracle_of(name)
    m = n + (TAIL if tail else 0)
    assert aux["tile_len"].shape == (1, 1) and aux["tile_len"][0, 0] == m and (aux["radii"] > 0).all()
    assert aux["n_contrib"].max() == n and not aux["saturated"].any()
    first = np.arange(m) < n
    ends = np.array(sorted({0, n - 1} | {i for i in (62, 63, 64, 65, 126, 127, 128) if i < n}))
    assert_above_floor(name, ends, ("opacity", "color", "mean2D"))
    g, _, r = run(backend, c)
    assert r.backward_rows()[0] == m
    if tail:
        assert_zero(g64, ~first, "the statement: a Gaussian under 1 / 255")
        assert_zero(g, ~first, "a Gaussian behind the wave's last contributor")
    judge(name, g, only=first)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_saturation_and_the_cap(backend):
    c = case("sat")
    g64, e32, pg32, aux = oracle_of("sat")
    sat_at, ncon = aux["sat_at"], aux["n_contrib"]
    assert aux["tile_len"].size <= 2 and aux["tile_len"].min() > 128
    early, late = (sat_at >= 0) & (sat_at < 64), sat_at >= 128
    assert early.sum() >= 8 and late.sum() >= 8, "pixels that saturate within the first batch and after the second"
    share = aux["capped"] / aux["contributing"]
    print(f"[sat] saturated within 64: {int(early.sum())} px, after 128: {int(late.sum())} px, not at all: "
          f"{int((sat_at < 0).sum())} px; cap share {share:.1%}")
    assert share >= 0.05
    # the Gaussians of c["behind"] come after every pixel's last contributor in both lists
    rect = aux["rect"][c["behind"]].astype(np.int64)
    assert (aux["radii"] > 0).all() and (rect == [0, 0, 2, 1]).all(), "the deepest Gaussians end both lists"
    for t in range(2):
        assert ncon[:, 16 * t:16 * t + 16].max() <= aux["tile_len"][0, t] - c["behind"].size
    assert aux["saturated"].all()
    assert_zero(g64, c["behind"], "the statement: a Gaussian behind every last contributor")
    front = np.arange(SAT_FRONT)
    capped = np.nonzero(aux["capped_of"] > 0)[0]
    slabs = capped[capped > SAT_FRONT + SAT_FAINT]
    assert (c["arrays"]["opacities"][slabs] == 1.0).all() and slabs.size >= 2 and aux["capped_of"][front].sum() > 0
    assert_above_floor("sat", front, ("opacity", "color", "mean2D", "mean3D"))
    assert_above_floor("sat", slabs, ("opacity", "color", "conic"))
    print(f"[sat] capped slabs {slabs.tolist()}: {aux['capped_of'][slabs].tolist()} evaluations; front: "
          f"{aux['capped_of'][front].tolist()}")
    g, _, _ = run(backend, c)
    assert_zero(g, c["behind"], "a Gaussian behind every pixel's last contributor")
    judge("sat", g)


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_everything_culled_writes_zeros(backend):
    c = case("culled")
    assert c["zeroed"] == 0
    aux = rs.render(rs.leaves(c["arrays"]), c["cam"], c["W"], c["H"], c["bg"], c["deg"])[1]
    assert not aux["radii"].any() and aux["tile_len"].max() == 0
    g, radii, r = run(backend, c)
    assert not radii.any()
    assert_zero(g, slice(None), "a scene with nothing to render")
    assert r.backward_rows()[0] == 0


def test_a_single_visible_gaussian(backend):
    aux = oracle_of("single")[3]
    assert aux["radii"][0] > 0 and aux["n_contrib"].max() == 1
    g, _, r = run(backend, case("single"))
    assert r.backward_rows()[0] == int(aux["tile_len"].astype(bool).sum())
    judge("single", g)


def test_no_gaussians_is_success(backend):
    c = case("single")
    empty = dict(c, arrays={k: (None if v is None else v[:0]) for k, v in c["arrays"].items()})
    g, radii, r = run(backend, empty)
    assert radii.shape == (0,) and all(v is None or v.shape[0] == 0 for v in g.values())
    assert r.backward_rows()[0] == 0


def test_zero_pixel_gradient_gives_zero_gradients(backend):
    c = case("size33x47")
    assert (oracle_of("size33x47")[3]["radii"] > 0).sum() >= 40
    g, _, _ = run(backend, c, w=np.zeros_like(c["w"]))
    assert_zero(g, slice(None), "dL_dpix = 0")


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_rows_of_an_earlier_backward_do_not_leak(backend):
    """the row arena is grow-only: after case 6 it holds non-zero rows where case 5's tail (rows no wave writes) lands"""
    first, second = case("sat"), case("list129_tail")
    aux1, aux2 = oracle_of("sat")[3], oracle_of("list129_tail")[3]
    rows1, rows2 = int(aux1["tile_len"].sum()), int(aux2["tile_len"].sum())
    assert rows1 >= rows2, "the second pass reuses rows the first one wrote"
    _, _, r = run(backend, first)
    assert r.backward_rows()[0] == rows1
    g_reused, _, _ = run(backend, second, r=r)
    assert r.backward_rows()[0] == rows2
    g_fresh, _, _ = run(backend, second)
    assert_bitwise(g_reused, g_fresh)
    assert_zero(g_reused, np.arange(129, 129 + TAIL), "a Gaussian whose rows no wave writes")


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_backward_after_an_overflowed_forward_is_an_error(backend):
    name = "sh3_16"
    c = case(name)
    aux = oracle_of(name)[3]
    a, cam = c["arrays"], c["cam"]
    d = lambda v: backend.dev(np.array(v))
    P = a["means3D"].shape[0]
    assert int(aux["tile_len"].sum()) > 8 * 64
    r = Rasterizer(0, lib=backend.lib)
    r.reserve(P, 1, c["W"], c["H"], 64)            # far too small on purpose
    args = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(c["bg"]), c["W"], c["H"], cam.tanfovx,
            cam.tanfovy)
    kw = dict(shs=d(a["shs"]), scales=d(a["scales"]), rotations=d(a["rotations"]), sh_degree=c["deg"])
    r.forward(d(a["means3D"]), d(a["opacities"]), *args, sync=False, **kw)
    with pytest.raises(RuntimeError, match="overflowed"):
        r.backward(d(c["w"]), d(a["means3D"]), *args, **kw)
    g, _, _ = run(backend, c, r=r)                 # synchronous forward: grows the arena and repeats
    assert r.backward_rows()[0] == int(aux["tile_len"].sum())
    judge(name, g, label=name + "/after overflow")
