"""PyTorch statement of the rasteriser's depth and opacity maps (gs2m_rasterize_depth, csrc/raster_depth.h): the oracle of
tests/test_raster_depth*.py.  Built like tests/raster_statement.py, whose projection it repeats without the autograd parts:
every (Gaussian, pixel) pair of a tile is evaluated densely, the three decisions of renderCUDA are masks, the global order is
(fp32 view-space depth, id).  Runs in fp64 (the oracle) or fp32 (the yardstick of the tolerance).  Not collected by pytest.

Per pixel, over the tile's list front to back, with alpha = min(0.99, o G) and an instance skipped where power > 0 or
alpha < 1/255:   T' = T (1 - alpha); the pixel is finished BEFORE accumulating the first instance with T' < 1e-4;
w = alpha T, S += w, Z += w z, T = T';  the median is the first contributor after which T <= 0.5.
    alpha = 1 - T        depth_expected = S > 0 ? Z / S : 0        depth_median = z of the median contributor, 0 without one
"""
import numpy as np
import torch

NEAR05_REL = 1e-4


def project(arrays, cam, W, H, scale_modifier=1.0, dtype=torch.float64):
    """raster_statement.render's projection (forward.cu:74-237) in ``dtype`` -> dict of mx, my, conic (ca, cb, cc), op, z
    (tensors [P]), depth32 (numpy fp32, the sort key), rect [P,4] and visible [P] (numpy)"""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    xyz = t(arrays["means3D"])
    P = xyz.shape[0]
    vm = torch.tensor(np.asarray(cam.world_view_transform, np.float64).reshape(16), dtype=dtype)
    pm = torch.tensor(np.asarray(cam.full_proj_transform, np.float64).reshape(16), dtype=dtype)
    tanx, tany = float(cam.tanfovx), float(cam.tanfovy)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if arrays.get("cov3D_precomp") is not None:
        c3 = t(arrays["cov3D_precomp"])
    else:
        s = scale_modifier * t(arrays["scales"])
        q = t(arrays["rotations"])
        r_, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r_ * qz), 2 * (qx * qz + r_ * qy)],
             [2 * (qx * qy + r_ * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r_ * qx)],
             [2 * (qx * qz - r_ * qy), 2 * (qy * qz + r_ * qx), 1 - 2 * (qx * qx + qy * qy)]]
        A = [[R[i][j] * s[:, j] for j in range(3)] for i in range(3)]
        S = [[sum(A[i][k] * A[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
        c3 = torch.stack([S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]], dim=1)
    V = [[c3[:, 0], c3[:, 1], c3[:, 2]], [c3[:, 1], c3[:, 3], c3[:, 4]], [c3[:, 2], c3[:, 4], c3[:, 5]]]
    tvx = vm[0] * x + vm[4] * y + vm[8] * z + vm[12]
    tvy = vm[1] * x + vm[5] * y + vm[9] * z + vm[13]
    tvz = vm[2] * x + vm[6] * y + vm[10] * z + vm[14]
    x32, y32, z32 = (v.to(torch.float32) for v in (x, y, z))
    v32 = vm.to(torch.float32)
    depth32 = (v32[2] * x32 + v32[6] * y32 + v32[10] * z32 + v32[14]).numpy()
    visible = depth32 > np.float32(0.2)
    hx = pm[0] * x + pm[4] * y + pm[8] * z + pm[12]
    hy = pm[1] * x + pm[5] * y + pm[9] * z + pm[13]
    hw = pm[3] * x + pm[7] * y + pm[11] * z + pm[15]
    p_w = 1.0 / (hw + 1e-7)
    ndc_x, ndc_y = hx * p_w, hy * p_w
    safe_z = torch.where(torch.from_numpy(visible), tvz, torch.ones_like(tvz))
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = tvx / safe_z, tvy / safe_z
    tx = torch.where((txtz < -limx) | (txtz > limx), txtz.clamp(-limx, limx) * safe_z, tvx)
    ty = torch.where((tytz < -limy) | (tytz > limy), tytz.clamp(-limy, limy) * safe_z, tvy)
    J00, J02 = fx / safe_z, -(fx * tx) / (safe_z * safe_z)
    J11, J12 = fy / safe_z, -(fy * ty) / (safe_z * safe_z)
    T0 = [vm[0] * J00 + vm[2] * J02, vm[4] * J00 + vm[6] * J02, vm[8] * J00 + vm[10] * J02]
    T1 = [vm[1] * J11 + vm[2] * J12, vm[5] * J11 + vm[6] * J12, vm[9] * J11 + vm[10] * J12]
    VT0 = [sum(V[i][k] * T0[k] for k in range(3)) for i in range(3)]
    VT1 = [sum(V[i][k] * T1[k] for k in range(3)) for i in range(3)]
    a = sum(T0[i] * VT0[i] for i in range(3)) + 0.3
    b = sum(T0[i] * VT1[i] for i in range(3))
    c = sum(T1[i] * VT1[i] for i in range(3)) + 0.3
    det = a * c - b * b
    visible &= (det != 0).numpy()
    ok_t = torch.from_numpy(visible)
    one = torch.ones_like(a)
    a_, b_, c_ = torch.where(ok_t, a, one), torch.where(ok_t, b, 0 * one), torch.where(ok_t, c, one)
    inv = 1.0 / (a_ * c_ - b_ * b_)
    ca, cb, cc = c_ * inv, -b_ * inv, a_ * inv
    mid = 0.5 * (a + c)
    root = torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
    radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + root, mid - root))).numpy().astype(np.int64)
    mx = ((ndc_x + 1.0) * W - 1.0) * 0.5
    my = ((ndc_y + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + 15) // 16, (H + 15) // 16
    mxn, myn = mx.numpy(), my.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        trunc = lambda v: np.trunc(np.where(np.isfinite(v), v, 0.0)).astype(np.int64)
        x0 = np.clip(trunc((mxn - radius) / 16.0), 0, gx)
        y0 = np.clip(trunc((myn - radius) / 16.0), 0, gy)
        x1 = np.clip(trunc((mxn + radius + 15) / 16.0), 0, gx)
        y1 = np.clip(trunc((myn + radius + 15) / 16.0), 0, gy)
    visible &= (x1 - x0) * (y1 - y0) > 0
    rect = np.stack([x0, y0, x1, y1], axis=1) * visible[:, None]
    return dict(mx=mx, my=my, ca=ca, cb=cb, cc=cc, op=t(arrays["opacities"]).reshape(-1), z=tvz, depth32=depth32, rect=rect,
                visible=visible, P=P)


def depth_maps(arrays, cam, W, H, scale_modifier=1.0, dtype=torch.float64):
    """-> dict of numpy [H,W] arrays: alpha, expected, median (float64 values of the ``dtype`` evaluation), median_id (index of
    the median's Gaussian, -1 = none), n_contrib (list position after the last contributor, 0 = none), near05 (some
    contributor leaves T within NEAR05_REL, relative, of 0.5: fp32 and fp64 may pick different medians) and tile_len[gy,gx]"""
    g = project(arrays, cam, W, H, scale_modifier, dtype)
    P, rect, visible = g["P"], g["rect"], g["visible"]
    order = np.lexsort((np.arange(P), g["depth32"]))
    order = order[visible[order]]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    out = dict(alpha=np.zeros((H, W)), expected=np.zeros((H, W)), median=np.zeros((H, W)),
               median_id=np.full((H, W), -1, np.int64), n_contrib=np.zeros((H, W), np.int64), near05=np.zeros((H, W), bool),
               tile_len=np.zeros((gy, gx), np.int64))
    for tyi in range(gy):
        for txi in range(gx):
            sel = order[(rect[order, 0] <= txi) & (txi < rect[order, 2]) & (rect[order, 1] <= tyi) & (tyi < rect[order, 3])]
            out["tile_len"][tyi, txi] = sel.size
            if sel.size == 0:
                continue
            ys, xs = np.meshgrid(np.arange(tyi * 16, min(tyi * 16 + 16, H)), np.arange(txi * 16, min(txi * 16 + 16, W)),
                                 indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            idx = torch.from_numpy(sel)
            dx = g["mx"][idx][:, None] - torch.tensor(xs, dtype=dtype)[None, :]
            dy = g["my"][idx][:, None] - torch.tensor(ys, dtype=dtype)[None, :]
            power = -0.5 * (g["ca"][idx][:, None] * dx * dx + g["cc"][idx][:, None] * dy * dy) - g["cb"][idx][:, None] * dx * dy
            alpha = torch.clamp_max(g["op"][idx][:, None] * torch.exp(torch.clamp_max(power, 0.0)), 0.99)
            valid = (power <= 0) & (alpha >= 1.0 / 255.0)
            a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
            sat = valid & (torch.cumprod(1.0 - a_eff, dim=0) < 1e-4)      # stop BEFORE accumulating the first such instance
            m = valid & ~(torch.cumsum(sat.to(torch.int64), dim=0) > 0)
            a_m = torch.where(m, alpha, torch.zeros_like(alpha))
            T_incl = torch.cumprod(1.0 - a_m, dim=0)
            T_excl = torch.cat([torch.ones_like(T_incl[:1]), T_incl[:-1]], dim=0)
            w = a_m * T_excl
            S = w.sum(dim=0)
            Z = (w * g["z"][idx][:, None]).sum(dim=0)
            pos = torch.arange(1, sel.size + 1)[:, None]
            half = m & (T_incl <= 0.5)
            first = torch.where(half, pos - 1, torch.full_like(pos, sel.size)).min(dim=0).values
            has = first < sel.size
            mid = idx[first.clamp_max(sel.size - 1)]
            out["alpha"][ys, xs] = (1.0 - T_incl[-1]).double().numpy()
            out["expected"][ys, xs] = torch.where(S > 0, Z / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S)).double().numpy()
            out["median"][ys, xs] = torch.where(has, g["z"][mid], torch.zeros_like(S)).double().numpy()
            out["median_id"][ys, xs] = torch.where(has, mid, torch.full_like(mid, -1)).numpy()
            out["n_contrib"][ys, xs] = (pos * m).max(dim=0).values.numpy()
            out["near05"][ys, xs] = (m & ((T_incl - 0.5).abs() <= NEAR05_REL * 0.5)).any(dim=0).numpy()
    return out


def errors(x, x64, keep):
    """(max|x - x64| / max|x64|, relative L2) over the kept pixels"""
    ref = np.asarray(x64, np.float64)[keep]
    d = np.asarray(x, np.float64)[keep] - ref
    return float(np.abs(d).max(initial=0.0) / np.abs(ref).max()), float(np.sqrt((d * d).sum() / (ref * ref).sum()))
