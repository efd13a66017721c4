"""The vote of gs2m_depth_consistency (include/gs2mesh_amd.h) in numpy: f32 arrays, one operation per line, so that every
intermediate is rounded to f32 on its own as the kernel's is.  The tests compare the kernel with this bit for bit, and
tests/test_depth_consistency_quality.py measures what the filter is for on this statement alone."""
import numpy as np

F = np.float32


def valid_map(depth, mask, min_depth, max_depth):
    d = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        ok = (d > F(0)) & (d >= F(min_depth)) & (d < F(max_depth))
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    return ok


def votes(depths, intrinsics, sources, pair, rel_tol, min_depth, max_depth, masks=None):
    """-> (valid, support, violation, occluded): lists of [H,W] arrays (bool, u8, u8, u8).  ``intrinsics[i]`` = (fx, fy, cx, cy);
    ``sources`` int [n,K] (-1 = none); ``pair`` f32 [n,K,12]."""
    n = len(depths)
    sources = np.asarray(sources, np.int64).reshape(n, -1)
    K = sources.shape[1]
    pair = np.asarray(pair, F).reshape(n, K, 12)
    masks = masks if masks is not None else [None] * n
    depths = [np.asarray(d, F) for d in depths]
    ok_all = [valid_map(depths[i], masks[i], min_depth, max_depth) for i in range(n)]
    out = []
    with np.errstate(all="ignore"):
        for i in range(n):
            D = depths[i]
            H, W = D.shape
            fx, fy, cx, cy = (F(v) for v in intrinsics[i])
            u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
            v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
            x = u - cx
            x = x * D
            x = x / fx
            y = v - cy
            y = y * D
            y = y / fy
            z = D
            sup = np.zeros((H, W), np.int32)
            vio = np.zeros((H, W), np.int32)
            occ = np.zeros((H, W), np.int32)
            for k in range(K):
                j = int(sources[i, k])
                if j < 0:
                    continue
                M = pair[i, k]
                q = []
                for r in range(3):
                    a = M[4 * r + 0] * x
                    b = M[4 * r + 1] * y
                    s = a + b
                    c = M[4 * r + 2] * z
                    s = s + c
                    s = s + M[4 * r + 3]
                    q.append(s.astype(F))
                q0, q1, q2 = q
                Dj = depths[j]
                Hj, Wj = Dj.shape
                fxj, fyj, cxj, cyj = (F(t) for t in intrinsics[j])
                vote = ok_all[i] & (q2 > F(0))
                pu = q0 * fxj
                pu = pu / q2
                pu = pu + cxj
                pu = pu + F(0.5)
                pv = q1 * fyj
                pv = pv / q2
                pv = pv + cyj
                pv = pv + F(0.5)
                vote = vote & (pu >= F(0)) & (pu < F(Wj)) & (pv >= F(0)) & (pv < F(Hj))
                iu = np.where(vote, np.floor(pu), F(0)).astype(np.int64)
                iv = np.where(vote, np.floor(pv), F(0)).astype(np.int64)
                vote = vote & ok_all[j][iv, iu]
                ds = Dj[iv, iu]
                diff = ds - q2
                tol = F(rel_tol) * q2
                is_sup = np.abs(diff) <= tol
                is_vio = ~is_sup & (diff > tol)
                is_occ = ~is_sup & ~is_vio
                sup += vote & is_sup
                vio += vote & is_vio
                occ += vote & is_occ
            out.append((ok_all[i], sup.astype(np.uint8), vio.astype(np.uint8), occ.astype(np.uint8)))
    return tuple([o[c] for o in out] for c in range(4))


def keep_maps(valid, support, violation, min_support, max_violation):
    return [(ok & (s.astype(np.int32) >= min_support) & (v.astype(np.int32) <= max_violation)).astype(np.uint8)
            for ok, s, v in zip(valid, support, violation)]


def consistency(depths, intrinsics, sources, pair, rel_tol, min_depth, max_depth, min_support, max_violation, masks=None):
    """-> (keep, support, violation, occluded), lists of [H,W] u8"""
    valid, sup, vio, occ = votes(depths, intrinsics, sources, pair, rel_tol, min_depth, max_depth, masks)
    return keep_maps(valid, sup, vio, min_support, max_violation), sup, vio, occ


# ---- the ring scene of the tests ----------------------------------------------------------------------------------------------
RING = dict(n=12, W=96, H=64, f=150.0, cx=48.0, cy=32.0, radius=0.6, rel_tol=0.01, min_depth=0.0, max_depth=100.0)


def ring_scene(noise=True):
    """12 views of the sphere on ``synthetic.ring_poses(12)``: dict(poses [n,3,4] world -> camera, camera_to_world [n,4,4], clean,
    depths (noisy), outlier (the injected pixels), intrinsics, sources (i+-1, i+-2), pair)."""
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.depth_utils import pair_matrices
    g = RING
    n, W, H = g["n"], g["W"], g["H"]
    poses = synthetic.ring_poses(n)
    c2w = []
    for p in poses:
        E = np.eye(4)
        E[:3] = p
        c2w.append(np.linalg.inv(E))
    c2w = np.stack(c2w)
    clean = [synthetic.sphere_depth(p, W, H, g["f"], g["f"], g["cx"], g["cy"], g["radius"]) for p in poses]
    rng = np.random.default_rng(7)
    depths, outlier = [], []
    for D in clean:
        m = (rng.random((H, W)) < 0.05) & (D > 0)
        side = rng.random((H, W)) < 0.5
        lo = rng.uniform(0.7, 0.95, (H, W))
        hi = rng.uniform(1.05, 1.3, (H, W))
        noisy = np.where(m, D * np.where(side, lo, hi), D).astype(np.float32)
        depths.append(noisy if noise else D)
        outlier.append(m)
    sources = np.array([[(i - 1) % n, (i + 1) % n, (i - 2) % n, (i + 2) % n] for i in range(n)], np.int32)
    return dict(poses=poses, camera_to_world=c2w, clean=clean, depths=depths, outlier=outlier,
                intrinsics=[(g["f"], g["f"], g["cx"], g["cy"])] * n, sources=sources, pair=pair_matrices(c2w, sources))
