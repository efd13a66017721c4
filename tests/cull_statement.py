"""The two statements gs2m_points_cull_views is tested against (evaluation/DTU/eval_code/evaluate_single_scene.py:63-99).

(a) ``keep_a``: the arithmetic of include/gs2mesh_amd.h in numpy f32, one rounded operation at a time, with the sampling done
    by torch's own ``F.grid_sample`` on the CPU -- so the sampling half is the reference's code, not a restatement.  The kernel
    must equal it exactly.
(b) ``keep_b``: the reference's lines literally -- ``intrinsic @ w2c @ vertices`` in torch f32 on the CPU, the 4 x 4 matrices
    from an RQ decomposition of P (numpy / scipy, standing where the reference calls cv2.decomposeProjectionMatrix), then
    ``grid_sample``.  Its matmul sums in the BLAS's order, so it agrees with (a) only away from the rounding boundaries.
"""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


def unnormalized(points, proj, norm_size, mask_size):
    """(a)'s coordinates for one view -> (gx, gy, tx, ty) f32 [V]: the grid coordinates and what grid_sample rounds,
    t = ((g + 1) / 2) * (size - 1)"""
    p = np.asarray(points, f32)
    m = np.asarray(proj, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        c = [((m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2]) + m[k, 3] for k in range(3)]
        den = c[2] + f32(1e-6)
        u, v = c[0] / den, c[1] / den
        gx = (u / (f32(norm_size[0]) - f32(1)) - f32(0.5)) * f32(2)
        gy = (v / (f32(norm_size[1]) - f32(1)) - f32(0.5)) * f32(2)
        tx = ((gx + f32(1)) / f32(2)) * f32(mask_size[0] - 1)
        ty = ((gy + f32(1)) / f32(2)) * f32(mask_size[1] - 1)
    assert all(a.dtype == f32 for a in (gx, gy, tx, ty))
    return gx, gy, tx, ty


def _sample(mask, gx, gy):
    """the reference's line 92 on one [H,W] 0 / 1 mask -> [V] f32"""
    maski = torch.from_numpy(np.ascontiguousarray(mask, f32))[None, None]
    pix = torch.from_numpy(np.stack([gx, gy], -1).astype(f32))
    return F.grid_sample(maski, pix[None, None], mode="nearest", padding_mode="zeros", align_corners=True)[0, -1, 0].numpy()


def keep_a(points, proj, masks, norm_size):
    """points [V,3], proj [n,3,4], masks [n,H,W] 0 / 1 -> bool [V]"""
    points = np.asarray(points, f32).reshape(-1, 3)
    keep = np.ones(len(points), bool)
    for i in range(len(proj)):
        H, W = masks[i].shape
        gx, gy, _, _ = unnormalized(points, proj[i], norm_size, (W, H))
        with np.errstate(invalid="ignore"):
            valid = (gx > -1) & (gx < 1) & (gy > -1) & (gy < 1)
        s = _sample(masks[i], gx, gy) if len(points) else np.zeros(0, f32)
        keep &= (s + (f32(1) - valid.astype(f32))) > 0
    return keep


def decompose(P):
    """P [3,4] -> (K [3,3] upper triangular with a positive diagonal, R [3,3], C [3]) with P = K [R | -R C]: what
    cv2.decomposeProjectionMatrix returns as (cameraMatrix, rotMatrix, transVect[:3] / transVect[3])"""
    from scipy.linalg import rq
    P = np.asarray(P, np.float64)
    K, R = rq(P[:, :3])
    S = np.diag(np.sign(np.diag(K)))
    K, R = K @ S, S @ R
    C = -np.linalg.solve(P[:, :3], P[:, 3])
    return K, R, C


def keep_b(points, world_mats, scale_mats, masks, norm_size):
    """the reference's cull_scan loop from the cameras' world_mat / scale_mat; ``masks`` are the already dilated [n,H,W]"""
    norm_w, norm_h = norm_size
    xyz = torch.from_numpy(np.asarray(points, np.float64))
    homog = torch.cat([xyz, torch.ones(len(xyz), 1, dtype=xyz.dtype)], dim=1).T.float()          # [4,V] f32, as :57-60
    per_view = []
    for wm, sm, mask in zip(world_mats, scale_mats, masks):
        P = (np.asarray(wm).astype(f32) @ np.asarray(sm).astype(f32))[:3, :4]                    # :34-35
        K, R, C = decompose(P)
        k4 = np.eye(4)                                                                           # the loader's 4 x 4 pair: K / K[2,2]
        k4[:3, :3] = K / K[2, 2]
        c2w = np.eye(4, dtype=f32)                                                               # and the camera-to-world pose
        c2w[:3, :3] = R.T
        c2w[:3, 3] = C
        w2c = torch.inverse(torch.from_numpy(c2w).float())                                       # :65
        cam = torch.from_numpy(k4).float() @ w2c @ homog                                         # :70, torch's f32 matmul
        pix = (cam[:2] / (cam[2][None] + 1e-6)).T.contiguous()                                   # :71-72
        pix[:, 0] /= norm_w - 1                                                                  # :73-75
        pix[:, 1] /= norm_h - 1
        g = (pix - 0.5) * 2
        inside = ((g > -1.0) & (g < 1.0)).all(dim=1).float()                                     # :76
        s = F.grid_sample(torch.from_numpy(np.ascontiguousarray(mask, f32))[None, None], g[None, None], mode="nearest",
                          padding_mode="zeros", align_corners=True)[0, 0, 0]                     # :92
        per_view.append(s + (1.0 - inside))                                                      # :94
    return (torch.stack(per_view, dim=1) > 0).all(dim=1).numpy()                                 # :96-99


def exact_pixels(points, world_mats, scale_mats, norm_size, mask_size):
    """the mask-grid coordinates of every point in every view in f64, from the f64 projection -> (tx, ty) [n,V]"""
    p = np.asarray(points, np.float64)
    tx, ty = [], []
    for wm, sm in zip(world_mats, scale_mats):
        P = (np.asarray(wm).astype(f32) @ np.asarray(sm).astype(f32))[:3, :4].astype(np.float64)
        M = P / np.linalg.norm(P[2, :3])
        c = p @ M[:, :3].T + M[:, 3]
        with np.errstate(all="ignore"):
            u, v = c[:, 0] / (c[:, 2] + 1e-6), c[:, 1] / (c[:, 2] + 1e-6)
        tx.append(u / (norm_size[0] - 1) * (mask_size[0] - 1))
        ty.append(v / (norm_size[1] - 1) * (mask_size[1] - 1))
    return np.stack(tx), np.stack(ty)
