"""PyTorch statement of the ray-Gaussian intersection depth maps (gs2m_rasterize_depth_ray, csrc/raster_depth_ray.h; the
definition is in include/gs2mesh_amd.h): the oracle of tests/test_raster_depth_ray*.py.  The walk and its weights are those of
tests/depth_statement.py (``project`` is reused as it is); what differs is the depth an instance has at a pixel:

    g = (s1 s2, s0 s2, s0 s1), gmax = max g_k;   w_k = (g_k / gmax) (column k of M), c_k = w_k . mu   (0 where !(gmax > 0))
    sz = sqrt(max(sum_k s_k^2 M[2][k]^2, 0)),  lo = max(z_c - 4 sz, 0.2),  hi = z_c + 4 sz
    r = (((2 px + 1) / W - 1) tanfovx, ((2 py + 1) / H - 1) tanfovy, 1)
    u_k = w_k . r,  num = sum c_k u_k,  den = sum u_k^2,  t = (den > 0 and num / den finite) ? num / den : z_c
    z_j(p) = min(max(t, lo), hi)

with M = W R(q), W the view rotation, mu the view-space mean, s = scale_modifier * scales.  Runs in fp64 (the oracle) or fp32 (the
yardstick of the tolerance).  Not collected by pytest.
"""
import numpy as np
import torch

import depth_statement as ds

GRAZING = 1e-3      # den / (sum_k |w_k|^2 |r|^2) below this: the ray lies within ~1.8 degrees of the disc's plane


def records(arrays, cam, scale_modifier, dtype, z_c):
    """-> w [P,3,3] (w[:, k] = w_k), c [P,3], lo [P], hi [P] in ``dtype``; z_c [P] = the view depth the walk carries"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    xyz, s, q = t(arrays["means3D"]), scale_modifier * t(arrays["scales"]), t(arrays["rotations"])
    vm = t(np.asarray(cam.world_view_transform, np.float64).reshape(16))
    r_, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r_ * qz), 2 * (qx * qz + r_ * qy)],
         [2 * (qx * qy + r_ * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r_ * qx)],
         [2 * (qx * qz - r_ * qy), 2 * (qy * qz + r_ * qx), 1 - 2 * (qx * qx + qy * qy)]]
    # M[a][k] = sum_j W[a][j] R[j][k], W[a][j] = vm[4 j + a]
    M = [[vm[a] * R[0][k] + vm[4 + a] * R[1][k] + vm[8 + a] * R[2][k] for k in range(3)] for a in range(3)]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    mu = [vm[a] * x + vm[4 + a] * y + vm[8 + a] * z + vm[12 + a] for a in range(3)]
    g = [s[:, 1] * s[:, 2], s[:, 0] * s[:, 2], s[:, 0] * s[:, 1]]
    gmax = torch.fmax(g[0], torch.fmax(g[1], g[2]))
    oriented = (gmax > 0) & torch.isfinite(gmax)
    safe = torch.where(oriented, gmax, torch.ones_like(gmax))
    zero = torch.zeros_like(gmax)
    w, c = [], []
    for k in range(3):
        f = g[k] / safe
        wk = [torch.where(oriented, f * M[a][k], zero) for a in range(3)]
        w.append(torch.stack(wk, dim=1))
        c.append(wk[0] * mu[0] + wk[1] * mu[1] + wk[2] * mu[2])
    a = [s[:, k] * M[2][k] for k in range(3)]
    var = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    sz = torch.sqrt(torch.fmax(var, zero))
    lo = torch.fmax(z_c - 4 * sz, torch.full_like(sz, 0.2))
    hi = z_c + 4 * sz
    return torch.stack(w, dim=1), torch.stack(c, dim=1), lo, hi


def pixel_rays(xs, ys, W, H, cam, dtype):
    rx = ((2 * torch.tensor(xs, dtype=dtype) + 1) / W - 1) * float(cam.tanfovx)
    ry = ((2 * torch.tensor(ys, dtype=dtype) + 1) / H - 1) * float(cam.tanfovy)
    return rx, ry


def ray_z(w, c, lo, hi, z_c, rx, ry):
    """z_j(p) [n, pixels] and the grazing measure den / (sum |w_k|^2 |r|^2) for records w [n,3,3], c [n,3], lo, hi, z_c [n]"""
    u = [w[:, k, 0][:, None] * rx[None, :] + w[:, k, 1][:, None] * ry[None, :] + w[:, k, 2][:, None] for k in range(3)]
    num = c[:, 0][:, None] * u[0] + c[:, 1][:, None] * u[1] + c[:, 2][:, None] * u[2]
    den = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    q = num / torch.where(den > 0, den, torch.ones_like(den))
    t = torch.where((den > 0) & torch.isfinite(q), q, z_c[:, None].expand_as(q))
    z = torch.minimum(torch.maximum(t, lo[:, None]), hi[:, None])
    w2 = (w * w).sum(dim=(1, 2))[:, None] * (rx * rx + ry * ry + 1)[None, :]
    sin2 = torch.where(w2 > 0, den / torch.where(w2 > 0, w2, torch.ones_like(w2)), torch.ones_like(den))
    return z, sin2


def depth_maps(arrays, cam, W, H, scale_modifier=1.0, dtype=torch.float64, centre=False):
    """-> dict of numpy [H,W] arrays: alpha, expected, median (float64 values of the ``dtype`` evaluation), median_id, n_contrib,
    near05, tile_len (as depth_statement.depth_maps) and grazing[H,W]: some contributor with a weight > 0 meets the pixel's ray
    within GRAZING of its plane.  ``centre``: the centre maps by the same code (z_j(p) = z_j), a check of the walk"""
    g = ds.project(arrays, cam, W, H, scale_modifier, dtype)
    P, rect, visible = g["P"], g["rect"], g["visible"]
    w_all, c_all, lo_all, hi_all = records(arrays, cam, scale_modifier, dtype, g["z"])
    order = np.lexsort((np.arange(P), g["depth32"]))
    order = order[visible[order]]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    out = dict(alpha=np.zeros((H, W)), expected=np.zeros((H, W)), median=np.zeros((H, W)),
               median_id=np.full((H, W), -1, np.int64), n_contrib=np.zeros((H, W), np.int64), near05=np.zeros((H, W), bool),
               grazing=np.zeros((H, W), bool), tile_len=np.zeros((gy, gx), np.int64))
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
            rx, ry = pixel_rays(xs, ys, W, H, cam, dtype)
            zray, sin2 = ray_z(w_all[idx], c_all[idx], lo_all[idx], hi_all[idx], g["z"][idx], rx, ry)
            if centre:
                zray = g["z"][idx][:, None].expand_as(zray)
            S = w.sum(dim=0)
            Z = (w * zray).sum(dim=0)
            pos = torch.arange(1, sel.size + 1)[:, None]
            half = m & (T_incl <= 0.5)
            first = torch.where(half, pos - 1, torch.full_like(pos, sel.size)).min(dim=0).values
            has = first < sel.size
            row = first.clamp_max(sel.size - 1)
            mid = idx[row]
            zmed = zray.gather(0, row[None, :])[0]
            out["alpha"][ys, xs] = (1.0 - T_incl[-1]).double().numpy()
            out["expected"][ys, xs] = torch.where(S > 0, Z / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S)).double().numpy()
            out["median"][ys, xs] = torch.where(has, zmed, torch.zeros_like(S)).double().numpy()
            out["median_id"][ys, xs] = torch.where(has, mid, torch.full_like(mid, -1)).numpy()
            out["n_contrib"][ys, xs] = (pos * m).max(dim=0).values.numpy()
            out["near05"][ys, xs] = (m & ((T_incl - 0.5).abs() <= ds.NEAR05_REL * 0.5)).any(dim=0).numpy()
            out["grazing"][ys, xs] = (m & (w > 0) & (sin2 < GRAZING)).any(dim=0).numpy()
    return out


def record_limits(arrays, cam, scale_modifier=1.0):
    """fp64 (lo, hi) of every Gaussian -> numpy [P] each"""
    g_z = torch.tensor(np.asarray(arrays["means3D"], np.float64))
    vm = np.asarray(cam.world_view_transform, np.float64).reshape(16)
    z_c = vm[2] * g_z[:, 0] + vm[6] * g_z[:, 1] + vm[10] * g_z[:, 2] + vm[14]
    _, _, lo, hi = records(arrays, cam, scale_modifier, torch.float64, z_c)
    return lo.numpy(), hi.numpy()


errors = ds.errors
