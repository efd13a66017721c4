"""Differentiable PyTorch statement of the rasteriser's image and its RAY depth maps: the oracle of the gradients through
the ray-Gaussian intersection depth (gs2m_rasterize_backward_depth_ray; the derivative is stated in include/gs2mesh_amd.h) in
tests/test_raster_depth_ray_backward*.py and tests/test_depth_ray_training.py.

Built as tests/depth_grad_statement.py is built -- raster_statement.py's differentiable projection, with that file's derivative
conventions, feeding depth_statement.py's walk -- with the depth of instance j at pixel p being
ray_depth_statement.ray_z on the records of ray_depth_statement.records RESTATED OVER LEAF TENSORS (that function builds its own
tensors): w_k, c_k, lo and hi stay in the graph of means3D, scales and rotations, and z_c is the graph's view-space z.  Two
points of the derivative are explicit here:
    * sz = sqrt(v), v = sum_k s_k^2 M[2][k]^2: where v == 0 the derivative through the square root is taken as 0 (autograd
      would give inf * 0);
    * everything else is autograd's: min / max pass the gradient to the operand they select, gmax is differentiated through
      (t is invariant under a common scaling of the records, so that adds zero), the median is a gather.
Runs in fp64 (the oracle) or fp32 (the yardstick of the tolerance).  Not collected by pytest.
"""
import numpy as np
import torch

import ray_depth_statement as rds
from depth_statement import NEAR05_REL
from raster_statement import ConicInverse, leaves, sh_colour  # noqa: F401  (leaves: re-exported for the tests)

NEAR_CLAMP_REL = 1e-4     # t within this (relative) of lo or hi: fp32 may take the other branch of the clamp


def records(s, R, vm, xyz):
    """ray_depth_statement.records over graph tensors: s [P,3] = scale_modifier * scales, R = the 3 x 3 list of [P] entries of
    R(q), vm [16], xyz [P,3].  -> w [P,3,3] (w[:, k] = w_k), c [P,3] and two functions (z_c [n], idx) -> lo / hi [n]"""
    M = [[vm[a] * R[0][k] + vm[4 + a] * R[1][k] + vm[8 + a] * R[2][k] for k in range(3)] for a in range(3)]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    mu = [vm[a] * x + vm[4 + a] * y + vm[8 + a] * z + vm[12 + a] for a in range(3)]
    g = [s[:, 1] * s[:, 2], s[:, 0] * s[:, 2], s[:, 0] * s[:, 1]]
    gmax = torch.fmax(g[0], torch.fmax(g[1], g[2]))
    oriented = (gmax.detach() > 0) & torch.isfinite(gmax.detach())
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
    pos = var.detach() > 0
    sz = torch.where(pos, torch.sqrt(torch.where(pos, var, torch.ones_like(var))), zero)   # d sqrt := 0 at var == 0
    lo = lambda zc, idx: torch.fmax(zc - 4 * sz[idx], torch.full_like(zc, 0.2))
    hi = lambda zc, idx: zc + 4 * sz[idx]
    return torch.stack(w, dim=1), torch.stack(c, dim=1), lo, hi


def quotient(w, c, z_c, rx, ry):
    """ray_z's t before the clamp, and where it is the quotient num / den (elsewhere it is z_c); no graph"""
    u = [w[:, k, 0][:, None] * rx[None, :] + w[:, k, 1][:, None] * ry[None, :] + w[:, k, 2][:, None] for k in range(3)]
    num = c[:, 0][:, None] * u[0] + c[:, 1][:, None] * u[1] + c[:, 2][:, None] * u[2]
    den = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    q = num / torch.where(den > 0, den, torch.ones_like(den))
    ok = (den > 0) & torch.isfinite(q)
    return torch.where(ok, q, z_c[:, None].expand_as(q)), ok


def render(p, cam, W, H, bg, sh_degree=3, scale_modifier=1.0, *, pixel_order_seed=None, transmittance_from_back=False,
           centre=False):
    """depth_grad_statement.render with z_j(p) of the ray maps where it has the centre's z: expected and median are those of
    gs2m_rasterize_depth_ray, in the graph of means3D, scales and rotations.  ``centre=True`` puts the centre's z back (a check
    of this file against depth_grad_statement).  p must hold scales and rotations.
    -> (image[3,H,W], expected[H,W], median[H,W], alpha[H,W], aux).  aux: depth_grad_statement's, and per pixel, over the
    contributors with a weight > 0: grazing (den / (sum |w_k|^2 |r|^2) < GRAZING), near_clamp (t within NEAR_CLAMP_REL of lo or
    hi), grazing_quotient / near_clamp_quotient (the same two restricted to
    contributors whose z_j(p) is, or may in fp32 be, the quotient), clamped (t outside [lo, hi]), floor_clamped (t below a lo that is the 0.2 floor), fallback (t = z_c for want of a
    quotient); per Gaussian clamp_hi_of / clamp_lo_of / floor_of / fallback_of / quotient_of [P]: such (instance, pixel) pairs."""
    xyz = p["means3D"]
    dt = xyz.dtype
    P = xyz.shape[0]
    vm = torch.tensor(np.asarray(cam.world_view_transform, np.float64).reshape(16), dtype=dt)
    pm = torch.tensor(np.asarray(cam.full_proj_transform, np.float64).reshape(16), dtype=dt)
    cp = torch.tensor(np.asarray(cam.camera_center, np.float64).reshape(3), dtype=dt)
    bgt = torch.tensor(np.asarray(bg, np.float64).reshape(3), dtype=dt)
    tanx, tany = float(cam.tanfovx), float(cam.tanfovy)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if p.get("cov3D_precomp") is not None:
        raise ValueError("a forward with cov3D_precomp has no ray depth")
    else:
        s = scale_modifier * p["scales"]
        q = p["rotations"]
        r_, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r_ * qz), 2 * (qx * qz + r_ * qy)],
             [2 * (qx * qy + r_ * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r_ * qx)],
             [2 * (qx * qz - r_ * qy), 2 * (qy * qz + r_ * qx), 1 - 2 * (qx * qx + qy * qy)]]
        A = [[R[i][j] * s[:, j] for j in range(3)] for i in range(3)]
        S3 = [[sum(A[i][k] * A[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
        c3 = torch.stack([S3[0][0], S3[0][1], S3[0][2], S3[1][1], S3[1][2], S3[2][2]], dim=1)
        c3.retain_grad()
    rec_w, rec_c, rec_lo, rec_hi = records(s, R, vm, xyz)
    V = [[c3[:, 0], c3[:, 1], c3[:, 2]], [c3[:, 1], c3[:, 3], c3[:, 4]], [c3[:, 2], c3[:, 4], c3[:, 5]]]
    tvx = vm[0] * x + vm[4] * y + vm[8] * z + vm[12]
    tvy = vm[1] * x + vm[5] * y + vm[9] * z + vm[13]
    tvz = vm[2] * x + vm[6] * y + vm[10] * z + vm[14]
    x32, y32, z32 = (t.detach().to(torch.float32) for t in (x, y, z))
    v32 = vm.to(torch.float32)
    depth32 = (v32[2] * x32 + v32[6] * y32 + v32[10] * z32 + v32[14]).numpy()
    visible = depth32 > np.float32(0.2)
    hx = pm[0] * x + pm[4] * y + pm[8] * z + pm[12]
    hy = pm[1] * x + pm[5] * y + pm[9] * z + pm[13]
    hw = pm[3] * x + pm[7] * y + pm[11] * z + pm[15]
    p_w = 1.0 / (hw + 1e-7)
    ndc_x = hx * p_w + p["means2D"][:, 0]
    ndc_y = hy * p_w + p["means2D"][:, 1]
    safe_z = torch.where(torch.from_numpy(visible), tvz, torch.ones_like(tvz))
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = tvx / safe_z, tvy / safe_z
    out_x, out_y = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    tx = torch.where(out_x, (txtz.clamp(-limx, limx) * safe_z).detach(), tvx)
    ty = torch.where(out_y, (tytz.clamp(-limy, limy) * safe_z).detach(), tvy)
    J00, J02 = fx / safe_z, -(fx * tx) / (safe_z * safe_z)
    J11, J12 = fy / safe_z, -(fy * ty) / (safe_z * safe_z)
    T0 = [vm[0] * J00 + vm[2] * J02, vm[4] * J00 + vm[6] * J02, vm[8] * J00 + vm[10] * J02]
    T1 = [vm[1] * J11 + vm[2] * J12, vm[5] * J11 + vm[6] * J12, vm[9] * J11 + vm[10] * J12]
    VT0 = [sum(V[i][k] * T0[k] for k in range(3)) for i in range(3)]
    VT1 = [sum(V[i][k] * T1[k] for k in range(3)) for i in range(3)]
    a = sum(T0[i] * VT0[i] for i in range(3)) + 0.3
    b = sum(T0[i] * VT1[i] for i in range(3))
    c = sum(T1[i] * VT1[i] for i in range(3)) + 0.3
    det = (a * c - b * b).detach()
    visible &= (det != 0).numpy()
    one = torch.ones_like(a)
    ok_t = torch.from_numpy(visible)
    ca, cb, cc = ConicInverse.apply(torch.where(ok_t, a, one), torch.where(ok_t, b, 0 * one), torch.where(ok_t, c, one))
    for t in (ca, cb, cc):
        t.retain_grad()
    with torch.no_grad():
        mid = 0.5 * (a + c)
        root = torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
        radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + root, mid - root))).numpy().astype(np.int64)
    mx = ((ndc_x + 1.0) * W - 1.0) * 0.5
    my = ((ndc_y + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + 15) // 16, (H + 15) // 16
    mxn, myn = mx.detach().numpy(), my.detach().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        trunc = lambda v: np.trunc(np.where(np.isfinite(v), v, 0.0)).astype(np.int64)
        x0 = np.clip(trunc((mxn - radius) / 16.0), 0, gx)
        y0 = np.clip(trunc((myn - radius) / 16.0), 0, gy)
        x1 = np.clip(trunc((mxn + radius + 15) / 16.0), 0, gx)
        y1 = np.clip(trunc((myn + radius + 15) / 16.0), 0, gy)
    visible &= (x1 - x0) * (y1 - y0) > 0
    rect = np.stack([x0, y0, x1, y1], axis=1) * visible[:, None]
    radii = np.where(visible, radius, 0).astype(np.int32)
    if p.get("colors_precomp") is not None:
        rgb = p["colors_precomp"]
    else:
        d = xyz - cp[None, :]
        d = d / torch.sqrt((d * d).sum(dim=1, keepdim=True))
        rgb = sh_colour(sh_degree, p["shs"], d)
        rgb.retain_grad()
    op = p["opacities"].reshape(-1)
    order = np.lexsort((np.arange(P), depth32))
    order = order[visible[order]]
    image = torch.zeros((3, H, W), dtype=dt)
    expected = torch.zeros((H, W), dtype=dt)
    median = torch.zeros((H, W), dtype=dt)
    amap = torch.zeros((H, W), dtype=dt)
    capped_of = np.zeros(P, np.int64)
    n_contrib = np.zeros((H, W), np.int64)
    median_pos = np.zeros((H, W), np.int64)
    median_id = np.full((H, W), -1, np.int64)
    near05 = np.zeros((H, W), bool)
    saturated = np.zeros((H, W), bool)
    tile_len = np.zeros((gy, gx), np.int64)
    flags = {k: np.zeros((H, W), bool) for k in ("grazing", "near_clamp", "clamped", "floor_clamped", "fallback", "grazing_quotient",
                                                    "near_clamp_quotient")}
    per_g = {k: np.zeros(P, np.int64) for k in ("clamp_hi_of", "clamp_lo_of", "floor_of", "fallback_of", "quotient_of")}
    for tyi in range(gy):
        for txi in range(gx):
            sel = order[(rect[order, 0] <= txi) & (txi < rect[order, 2]) & (rect[order, 1] <= tyi) & (tyi < rect[order, 3])]
            ys, xs = np.meshgrid(np.arange(tyi * 16, min(tyi * 16 + 16, H)), np.arange(txi * 16, min(txi * 16 + 16, W)), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            if pixel_order_seed is not None:
                perm = np.random.default_rng([pixel_order_seed, tyi, txi]).permutation(ys.size)
                ys, xs = ys[perm], xs[perm]
            tile_len[tyi, txi] = sel.size
            if sel.size == 0:
                image[:, ys, xs] = bgt[:, None].expand(3, ys.size)
                continue
            idx = torch.from_numpy(sel)
            dx = mx[idx][:, None] - torch.tensor(xs, dtype=dt)[None, :]
            dy = my[idx][:, None] - torch.tensor(ys, dtype=dt)[None, :]
            power = -0.5 * (ca[idx][:, None] * dx * dx + cc[idx][:, None] * dy * dy) - cb[idx][:, None] * dx * dy
            G = torch.exp(torch.clamp_max(power, 0.0))
            alpha_raw = op[idx][:, None] * G
            alpha = alpha_raw + (torch.clamp_max(alpha_raw, 0.99) - alpha_raw).detach()   # straight-through cap
            valid = (power <= 0) & (alpha >= 1.0 / 255.0)
            a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
            sat = valid & (torch.cumprod(1.0 - a_eff, dim=0).detach() < 1e-4)   # stop BEFORE accumulating the first such instance
            m = valid & ~(torch.cumsum(sat.to(torch.int64), dim=0) > 0)
            a_m = torch.where(m, alpha, torch.zeros_like(alpha))
            T_incl = torch.cumprod(1.0 - a_m, dim=0)
            if transmittance_from_back:
                T_excl = T_incl[-1][None, :] / torch.flip(torch.cumprod(torch.flip(1.0 - a_m, [0]), dim=0), [0])
            else:
                T_excl = torch.cat([torch.ones_like(T_incl[:1]), T_incl[:-1]], dim=0)
            wgt = a_m * T_excl
            image[:, ys, xs] = (rgb[idx].t()[:, :, None] * wgt[None, :, :]).sum(dim=1) + T_incl[-1][None, :] * bgt[:, None]
            zc = tvz[idx]
            lo_s, hi_s = rec_lo(zc, idx), rec_hi(zc, idx)
            rx, ry = rds.pixel_rays(xs, ys, W, H, cam, dt)
            zs, sin2 = rds.ray_z(rec_w[idx], rec_c[idx], lo_s, hi_s, zc, rx, ry)
            if centre:
                zs = zc[:, None].expand_as(zs)
            with torch.no_grad():      # which branch every (instance, pixel) took: the masks and shares of the tests
                t_raw, quot = quotient(rec_w[idx], rec_c[idx], zc, rx, ry)
                on = m & (wgt > 0)
                above, below = t_raw > hi_s[:, None], t_raw < lo_s[:, None]
                floor = below & ~(lo_s > 0.2)[:, None]
                near = ((t_raw - lo_s[:, None]).abs() <= NEAR_CLAMP_REL * lo_s[:, None].abs()) | \
                       ((t_raw - hi_s[:, None]).abs() <= NEAR_CLAMP_REL * hi_s[:, None].abs())
                flags["grazing"][ys, xs] = (on & (sin2 < rds.GRAZING)).any(dim=0).numpy()
                flags["near_clamp"][ys, xs] = (on & near).any(dim=0).numpy()
                # the same two where the quotient is what z_j(p) depends on: a clamp that binds away from its threshold gives lo
                # or hi whatever digits t lost, and the fallback's t is z_c itself
                flags["grazing_quotient"][ys, xs] = (on & (sin2 < rds.GRAZING) & quot & ~above & ~below).any(dim=0).numpy()
                flags["near_clamp_quotient"][ys, xs] = (on & near & quot).any(dim=0).numpy()
                flags["clamped"][ys, xs] = (on & (above | below)).any(dim=0).numpy()
                flags["floor_clamped"][ys, xs] = (on & floor).any(dim=0).numpy()
                flags["fallback"][ys, xs] = (on & ~quot).any(dim=0).numpy()
                per_g["clamp_hi_of"][sel] += (on & above).sum(dim=1).numpy()
                per_g["clamp_lo_of"][sel] += (on & below & ~floor).sum(dim=1).numpy()
                per_g["floor_of"][sel] += (on & floor).sum(dim=1).numpy()
                per_g["fallback_of"][sel] += (on & ~quot & ~above & ~below).sum(dim=1).numpy()
                per_g["quotient_of"][sel] += (on & quot & ~above & ~below).sum(dim=1).numpy()
            S = wgt.sum(dim=0)
            Z = (wgt * zs).sum(dim=0)
            has_s = S.detach() > 0
            expected[ys, xs] = torch.where(has_s, Z / torch.where(has_s, S, torch.ones_like(S)), torch.zeros_like(S))
            amap[ys, xs] = 1.0 - T_incl[-1]
            pos = torch.arange(1, sel.size + 1)[:, None]
            half = m & (T_incl.detach() <= 0.5)
            first = torch.where(half, pos - 1, torch.full_like(pos, sel.size)).min(dim=0).values
            has = first < sel.size
            first_c = first.clamp_max(sel.size - 1)
            median[ys, xs] = torch.where(has, zs.gather(0, first_c[None, :])[0], torch.zeros_like(S))
            median_pos[ys, xs] = torch.where(has, first + 1, torch.zeros_like(first)).numpy()
            median_id[ys, xs] = torch.where(has, idx[first_c], torch.full_like(first, -1)).numpy()
            near05[ys, xs] = (m & ((T_incl.detach() - 0.5).abs() <= NEAR05_REL * 0.5)).any(dim=0).numpy()
            n_contrib[ys, xs] = (pos * m).max(dim=0).values.numpy()
            saturated[ys, xs] = sat.any(dim=0).numpy()
            capped_of[sel] += (m & (alpha_raw.detach() > 0.99)).sum(dim=1).numpy()
    aux = dict(radii=radii, rect=rect.astype(np.uint32), visible=visible, t_rgb=rgb, t_conic=(ca, cb, cc), t_cov3=c3,
               n_contrib=n_contrib, median_pos=median_pos, median_id=median_id, near05=near05, saturated=saturated,
               tile_len=tile_len, capped_of=capped_of, capped=int(capped_of.sum()), z=tvz.detach().numpy(), **flags, **per_g)
    return image, expected, median, amap, aux


def grads(arrays, cam, W, H, bg, deg, mod, weight_sets, dtype, **render_kw):
    """weight_sets: list (or a function aux -> list) of dicts of numpy wC[3,H,W], wD, wM, wA [H,W] (a missing / None entry = the term is absent).  One
    evaluation of the statement, one differentiation per set.  -> (list of dicts of fp64 numpy gradients keyed as
    Rasterizer.backward's, one per set, of loss = sum(wC image + wD expected_ray + wM median_ray + wA alpha); maps = (image, expected,
    median, alpha) as numpy; aux)"""
    p = leaves(arrays, dtype)
    maps = render(p, cam, W, H, bg, deg, mod, **render_kw)
    aux = maps[4]
    if callable(weight_sets):      # the masks of the weights come from this evaluation's own flags
        weight_sets = weight_sets(aux)
    P = np.asarray(arrays["means3D"]).shape[0]
    ca, cb, cc = aux["t_conic"]
    wrt = dict(mean2D=p["means2D"], ca=ca, cb=cb, cc=cc, opacity=p["opacities"], color=aux["t_rgb"], mean3D=p["means3D"],
               cov3D=aux["t_cov3"], sh=p.get("shs"), scale=p.get("scales"), rot=p.get("rotations"))
    names = [k for k, v in wrt.items() if v is not None]
    out = []
    for n, weights in enumerate(weight_sets):
        loss = 0
        for key, m in zip(("wC", "wD", "wM", "wA"), maps[:4]):
            if weights.get(key) is not None:
                loss = loss + (m * torch.tensor(weights[key], dtype=dtype)).sum()
        got = torch.autograd.grad(loss, [wrt[k] for k in names], retain_graph=n + 1 < len(weight_sets), allow_unused=True)
        r = {k: (np.zeros(tuple(wrt[k].shape), np.float64) if t is None else t.detach().numpy().astype(np.float64))
             for k, t in zip(names, got)}
        g = dict(mean2D=r["mean2D"], opacity=r["opacity"], color=r["color"], mean3D=r["mean3D"], cov3D=r["cov3D"],
                 conic=np.stack([r["ca"], 0.5 * r["cb"], np.zeros(P), r["cc"]], axis=1),   # dL_dconic.y is half the derivative
                 sh=r.get("sh"), scale=r.get("scale", np.zeros((P, 3))), rot=r.get("rot", np.zeros((P, 4))))
        out.append(g)
    return out, tuple(m.detach().numpy() for m in maps[:4]), aux
