"""Plain numpy statement of ``gs2m_stereo_sgm`` (include/gs2mesh_amd.h, steps 1-7): the matcher's reference in the tests.
Written from the statement, not from the kernels: it materialises the cost volume and walks the paths pixel by pixel.
Holds several [H,W,D] int32 arrays (about 1 GB at 640 x 480, D = 128): not for larger inputs.  Not collected by pytest."""
import numpy as np


def grey(rgb8):
    c = np.asarray(rgb8).astype(np.int32)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def census(g, wx=4, wy=3):
    H, W = g.shape
    p = np.pad(g, ((wy, wy), (wx, wx)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for dy in range(-wy, wy + 1):
        for dx in range(-wx, wx + 1):
            if dy == 0 and dx == 0:
                continue
            out = (out << np.uint64(1)) | (p[wy + dy:wy + dy + H, wx + dx:wx + dx + W] < g).astype(np.uint64)
    return out


def popcount(a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.int32)


def cost_volume(cl, cr, D, oob=62):
    H, W = cl.shape
    C = np.full((H, W, D), oob, np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount(cl[:, d:] ^ cr[:, :W - d])
    return C


def aggregate(C, dy, dx, P1, P2):
    """L_r of the path that steps by (dy, dx)"""
    H, W, D = C.shape
    L = np.zeros_like(C)
    big = 10 ** 6
    if dx == 0:
        steps = [(slice(y, y + 1), slice(None)) for y in (range(H) if dy > 0 else range(H - 1, -1, -1))]
    else:
        steps = [(slice(None), slice(x, x + 1)) for x in (range(W) if dx > 0 else range(W - 1, -1, -1))]
    prev = None
    for sl in steps:
        c = C[sl]
        if prev is None:
            cur = c.copy()
        else:
            m = prev.min(-1, keepdims=True)
            lo = np.concatenate([np.full_like(prev[..., :1], big), prev[..., :-1]], -1) + P1
            hi = np.concatenate([prev[..., 1:], np.full_like(prev[..., :1], big)], -1) + P1
            cur = c + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + P2)) - m
        L[sl] = cur
        prev = cur
    return L


def sgm_grey(gl, gr, D, P1=10, P2=120):
    """left-based matcher on two grey images (int32): (disp f32 [H,W], S int32 [H,W,D])"""
    C = cost_volume(census(gl), census(gr), D)
    S = np.zeros_like(C)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        S += aggregate(C, dy, dx, P1, P2)
    d = S.argmin(-1)
    H, W = d.shape
    yy, xx = np.mgrid[:H, :W]
    s0 = S[yy, xx, d].astype(np.float32)
    sm = S[yy, xx, np.clip(d - 1, 0, D - 1)].astype(np.float32)
    sp = S[yy, xx, np.clip(d + 1, 0, D - 1)].astype(np.float32)
    den = sm + sp - np.float32(2) * s0
    ok = (d > 0) & (d < D - 1) & (den > 0)
    sub = np.where(ok, (sm - sp) / np.where(ok, np.float32(2) * den, np.float32(1)), np.float32(0)).astype(np.float32)
    return (d.astype(np.float32) + sub).astype(np.float32), S


def sgm(left_rgb8, right_rgb8, D, P1=10, P2=120):
    """-> (disp_lr, disp_rl, S_lr): step 7 by the reference's protocol (flip both, swap, match, flip back)"""
    gl, gr = grey(left_rgb8), grey(right_rgb8)
    lr, S = sgm_grey(gl, gr, D, P1, P2)
    rl = sgm_grey(gr[:, ::-1], gl[:, ::-1], D, P1, P2)[0][:, ::-1]
    return lr, np.ascontiguousarray(rl), S


def occlusion(L2R, R2L, thr):
    """Stereo.get_occlusion_mask (True = visible)"""
    H, W = L2R.shape
    xg, yg = np.meshgrid(np.arange(W), np.arange(H))
    xp = (xg - L2R).astype(np.int32)
    xc = np.clip(xp, 0, W - 1)
    xr = np.clip(xc + R2L[yg, xc], 0, W - 1)
    m = np.abs(xg - xr) > thr
    m[(xp < 0) | (xp >= W)] = True
    return ~m
