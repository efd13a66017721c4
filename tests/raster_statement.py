"""Differentiable PyTorch statement of the reference rasteriser's forward (DGR/cuda_rasterizer/forward.cu): the oracle of the
backward pass in the tests.  Written from the statement in SURVEY.md Appendix A, not from the kernels: every (Gaussian, pixel)
pair of a tile is evaluated densely, the three decisions of renderCUDA are masks, and autograd supplies the derivative.
Runs in fp64 (the oracle) or fp32 (the yardstick of the tolerance).  Not collected by pytest.

Inputs are ACTIVATED parameters.  Sigma, the EWA cov2D + 0.3, the conic, the radius and the tile rect are computed here; the
rect only masks and is not differentiated.  The global order is (view-space depth, id) with the depth evaluated in fp32, as
the reference's sort keys are.

The reference's backward departs from the true derivative of its forward in a few places; its gradients are the contract,
so the departures are written into the statement:
  * min(0.99, o G): the cap acts on the value only, the derivative passes straight through (backward.cu:499, :541);
  * the conic inverse is a custom Function whose backward uses 1 / (det^2 + 1e-7) (backward.cu:203);
  * where tx / tz or ty / tz was clamped to 1.3 tan(fov), t.x / t.y is a constant (x_grad_mul / y_grad_mul, :175-176);
  * clamped SH channels pass no gradient (torch's clamp rule, :32-34);
  * `means2D` is an additive dummy in NDC space, so its gradient has the reference's 0.5 W / 0.5 H scaling (:460-461);
  * the background enters as C + T_final * bg (:531-534 is its derivative).
"""
import numpy as np
import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]


class ConicInverse(torch.autograd.Function):
    """(a, b, c) -> (c, -b, a) / det; backward as the reference writes it, with denom2inv = 1 / (det^2 + 1e-7)."""

    @staticmethod
    def forward(ctx, a, b, c):
        det = a * c - b * b
        ctx.save_for_backward(a, b, c, det)
        inv = 1.0 / det
        return c * inv, -b * inv, a * inv

    @staticmethod
    def backward(ctx, gA, gB, gC):
        a, b, c, det = ctx.saved_tensors
        gB = 0.5 * gB   # the reference's dL_dconic.y is HALF the derivative by conic.y (backward.cu:550), its formulas expect that
        d2i = 1.0 / (det * det + 1e-7)
        da = d2i * (-c * c * gA + 2 * b * c * gB + (det - a * c) * gC)
        dc = d2i * (-a * a * gC + 2 * a * b * gB + (det - a * c) * gA)
        db = d2i * 2 * (b * c * gA - (det + 2 * b * b) * gB + a * b * gC)
        return da, db, dc


def sh_colour(deg, sh, d):
    """forward.cu:20-71; sh [P,M,3], d [P,3] unit directions -> clamped rgb [P,3]"""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    r = SH_C0 * sh[:, 0]
    if deg > 0:
        r = r - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = r + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * sh[:, 6] \
                + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8]
            if deg > 2:
                r = r + SH_C3[0] * y * (3 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10] \
                    + SH_C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12] \
                    + SH_C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14] \
                    + SH_C3[6] * x * (xx - 3 * yy) * sh[:, 15]
    return torch.clamp_min(r + 0.5, 0.0)


def leaves(arrays, dtype=torch.float64):
    """dict of numpy arrays (None allowed) -> dict of leaf tensors that require grad, plus the `means2D` dummy"""
    out = {k: (None if v is None else torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True))
           for k, v in arrays.items()}
    P = np.asarray(arrays["means3D"]).shape[0]
    out["means2D"] = torch.zeros((P, 3), dtype=dtype, requires_grad=True)
    return out


def render(p, cam, W, H, bg, sh_degree=3, scale_modifier=1.0, *, clamp_passes_gradient=False, pixel_order_seed=None,
           transmittance_from_back=False):
    """p: dict of tensors means3D[P,3], opacities[P], means2D[P,3] (dummy), shs[P,M,3] | colors_precomp[P,3],
    scales[P,3] + rotations[P,4] | cov3D_precomp[P,6].  cam: graphics.Camera.  -> (image[3,H,W], aux dict of numpy arrays:
    radii[P], rect[P,4], capped = number of (Gaussian, pixel) evaluations that contributed with the 0.99 cap binding, and
    the intermediate tensors t_rgb, t_conic, t_cov3, whose .grad is filled by backward()).
    What the edge tests assert their purpose on: per pixel n_contrib[H,W] (position in the tile's list after the last
    contributor, 0 = none), saturated[H,W] and sat_at[H,W] (list position of the instance that would have taken T below 1e-4,
    -1 = none); per tile tile_len[gy,gx]; per Gaussian clamped_x / clamped_y[P] (t.x / t.y clamped to the 1.3 tan(fov)
    frustum), rgb_clamped[P,3] and capped_of[P] (evaluations of the Gaussian that contributed with the cap binding);
    contributing = number of contributing (Gaussian, pixel) evaluations.
    clamp_passes_gradient=True makes the clamped t.x / t.y differentiable: the WRONG derivative (not the reference's), there
    only so that a test can assert that its case tells the two apart.
    pixel_order_seed: the pixels of every tile are visited in a seeded random order instead of row by row.  The function is the
    same; what changes is the order in which a Gaussian's gradient is summed over its contributing pixels, so several seeds in
    fp32 show how far rounding alone moves a gradient (the yardstick of an ill-conditioned sum).
    transmittance_from_back: T in front of a contributor is T_final divided by the (1 - alpha) of every contributor from it to
    the last, multiplied up from the BACK of the list -- the order of the reference's backward (T = T / (1 - alpha),
    backward.cu:503) -- instead of the product from the front.  The same function again; in fp32 the FRONT of a long list now
    carries the rounding of the whole chain, as it does in any backward that rebuilds T that way."""
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
    # ---- Sigma (forward.cu:118-152)
    if p.get("cov3D_precomp") is not None:
        c3 = p["cov3D_precomp"]
    else:
        s = scale_modifier * p["scales"]
        q = p["rotations"]
        r_, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r_ * qz), 2 * (qx * qz + r_ * qy)],
             [2 * (qx * qy + r_ * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r_ * qx)],
             [2 * (qx * qz - r_ * qy), 2 * (qy * qz + r_ * qx), 1 - 2 * (qx * qx + qy * qy)]]
        A = [[R[i][j] * s[:, j] for j in range(3)] for i in range(3)]
        S = [[sum(A[i][k] * A[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
        c3 = torch.stack([S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]], dim=1)
        c3.retain_grad()
    # the six stored entries; the off-diagonal ones appear twice in the matrix (so their gradient counts both, as the reference's)
    V = [[c3[:, 0], c3[:, 1], c3[:, 2]], [c3[:, 1], c3[:, 3], c3[:, 4]], [c3[:, 2], c3[:, 4], c3[:, 5]]]
    # ---- view space, near cull, projection (forward.cu:186-205); the sort key is the fp32 depth
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
    # ---- EWA cov2D + 0.3 (forward.cu:74-113); clamped t.x / t.y are constants (backward.cu:175-176)
    safe_z = torch.where(torch.from_numpy(visible), tvz, torch.ones_like(tvz))
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = tvx / safe_z, tvy / safe_z
    out_x, out_y = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    cl_x, cl_y = txtz.clamp(-limx, limx) * safe_z, tytz.clamp(-limy, limy) * safe_z
    if clamp_passes_gradient:   # the derivative of min / max as if t.x / t.z alone had been clamped: NOT the contract
        cl_x, cl_y = cl_x.detach() + (tvx - tvx.detach()), cl_y.detach() + (tvy - tvy.detach())
    else:
        cl_x, cl_y = cl_x.detach(), cl_y.detach()
    tx = torch.where(out_x, cl_x, tvx)
    ty = torch.where(out_y, cl_y, tvy)
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
    # ---- radius and tile rect (forward.cu:220-237): masks only
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
    # ---- colour (forward.cu:20-71)
    if p.get("colors_precomp") is not None:
        rgb = p["colors_precomp"]
    else:
        d = xyz - cp[None, :]
        d = d / torch.sqrt((d * d).sum(dim=1, keepdim=True))
        rgb = sh_colour(sh_degree, p["shs"], d)
        rgb.retain_grad()
    op = p["opacities"].reshape(-1)
    # ---- compositing (forward.cu:261-374), tile by tile, in the global (depth, id) order
    order = np.lexsort((np.arange(P), depth32))
    order = order[visible[order]]
    image = torch.zeros((3, H, W), dtype=dt)
    capped = contributing = 0
    capped_of = np.zeros(P, np.int64)
    n_contrib = np.zeros((H, W), np.int64)
    sat_at = np.full((H, W), -1, np.int64)
    tile_len = np.zeros((gy, gx), np.int64)
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
            pxs = torch.tensor(xs, dtype=dt)[None, :]
            pys = torch.tensor(ys, dtype=dt)[None, :]
            dx = mx[idx][:, None] - pxs
            dy = my[idx][:, None] - pys
            power = -0.5 * (ca[idx][:, None] * dx * dx + cc[idx][:, None] * dy * dy) - cb[idx][:, None] * dx * dy
            G = torch.exp(torch.clamp_max(power, 0.0))
            alpha_raw = op[idx][:, None] * G
            alpha = alpha_raw + (torch.clamp_max(alpha_raw, 0.99) - alpha_raw).detach()   # straight-through cap
            valid = (power <= 0) & (alpha >= 1.0 / 255.0)
            a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
            one_minus = 1.0 - a_eff
            T_incl = torch.cumprod(one_minus, dim=0)
            T_excl = torch.cat([torch.ones_like(T_incl[:1]), T_incl[:-1]], dim=0)
            # stop BEFORE accumulating the first instance that would take T below 1e-4 (forward.cu:345-350); T_excl is the
            # true T up to and including that instance, which is all the test needs
            sat = valid & (T_incl.detach() < 1e-4)
            done = torch.cumsum(sat.to(torch.int64), dim=0) > 0
            m = valid & ~done
            a_m = torch.where(m, alpha, torch.zeros_like(alpha))
            Tm_incl = torch.cumprod(1.0 - a_m, dim=0)
            if transmittance_from_back:
                Tm_excl = Tm_incl[-1][None, :] / torch.flip(torch.cumprod(torch.flip(1.0 - a_m, [0]), dim=0), [0])
            else:
                Tm_excl = torch.cat([torch.ones_like(Tm_incl[:1]), Tm_incl[:-1]], dim=0)
            wgt = a_m * Tm_excl                                      # [n, px]
            col = (rgb[idx].t()[:, :, None] * wgt[None, :, :]).sum(dim=1) + Tm_incl[-1][None, :] * bgt[:, None]
            image[:, ys, xs] = col
            cap_here = m & (alpha_raw.detach() > 0.99)
            capped += int(cap_here.sum())
            capped_of[sel] += cap_here.sum(dim=1).numpy()
            contributing += int(m.sum())
            pos = torch.arange(1, sel.size + 1)[:, None]
            n_contrib[ys, xs] = (pos * m).max(dim=0).values.numpy()
            first_sat = torch.where(sat, pos - 1, torch.full_like(pos, sel.size)).min(dim=0).values.numpy()
            sat_at[ys, xs] = np.where(first_sat < sel.size, first_sat, -1)
            del T_excl
    rgb_clamped = np.zeros((P, 3), bool) if p.get("colors_precomp") is not None else (rgb.detach() <= 0).numpy()
    return image, dict(radii=radii, rect=rect.astype(np.uint32), capped=capped, visible=visible, t_rgb=rgb, t_conic=(ca, cb, cc),
                       t_cov3=c3, n_contrib=n_contrib, saturated=sat_at >= 0, sat_at=sat_at, tile_len=tile_len,
                       clamped_x=out_x.numpy() & visible, clamped_y=out_y.numpy() & visible, rgb_clamped=rgb_clamped,
                       contributing=contributing, capped_of=capped_of)
