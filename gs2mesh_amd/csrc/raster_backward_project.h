// raster_backward_project.h -- per-Gaussian half of the rasteriser's backward pass (the reference's computeCov2DCUDA,
// backward.cu:144-274, and preprocessCUDA, :347-396).  Part of the projection translation unit (-ffp-contract=off): the
// recomputed Sigma and projection are the forward's own functions in the forward's own translation unit; the SH clamp flags are
// read back from the colour the forward stored in the record.
//
//   k_bw_area_block_sums / k_bw_scan_blocks / k_bw_row_offsets: exclusive scan of the tile-rect areas of the projected records
//     -> row_offset[g], the first row of Gaussian g in the instance-row buffer (raster_backward_blend.h);
//   k_gaussian_backward: one thread per Gaussian.  Sums the Gaussian's rows in slot order (fixed order: bitwise reproducible),
//     then continues conic -> cov2D -> cov3D -> scale / rotation, mean2D -> mean3D (projection and cov2D's Jacobian) and
//     colour -> SH coefficients and, through the view direction, mean3D.  Sigma is recomputed from the inputs, the SH clamp flags
//     come from the record's colour.  Every output row is written; Gaussians the forward culled (radius 0) get zeros.
//
// Departures of the reference's backward from the true derivative, reproduced here (they are the contract):
//   * denom2inv = 1 / (denom^2 + 1e-7) in the derivative of the conic inverse (backward.cu:203);
//   * x_grad_mul / y_grad_mul: no gradient to t.x / t.y where the forward clamped them to the 1.3 tan(fov) frustum (:175-176);
//   * clamped SH channels (colour < 0 -> 0) pass no gradient (:32-34);
//   * dL/dmean2D stays in the NDC-scaled units the compositing accumulated, as [P,3] with z = 0 (:460-461).
// The gradients through the depth maps enter here as dL/dalpha already folded into the first nine row values, plus row[9].
// One difference FROM the reference: dL/dscale carries the factor scale_modifier (the true derivative of Sigma = R (mod s)^2 R^T);
// the reference's computeCov3D omits it (:321-325).  Identical at scale_modifier = 1, the only value training uses.
#pragma once
#include "raster_project.h"
#include "raster_internal.h"   // BwOut

GS2M_DEVICE unsigned bw_rect_area(const float4 c) {
    const unsigned rect0 = __float_as_uint(c.z), rect1 = __float_as_uint(c.w);
    const unsigned x0 = rect0 & 0xffffu, y0 = rect0 >> 16, x1 = rect1 & 0xffffu, y1 = rect1 >> 16;
    return (x1 > x0 && y1 > y0) ? (x1 - x0) * (y1 - y0) : 0u;
}

// exclusive scan of 256 values over one workgroup; returns this thread's prefix, *total = the workgroup's sum
GS2M_DEVICE unsigned bw_block_exclusive_scan(unsigned v, unsigned* s_w, unsigned* total) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const unsigned inc = wave_inclusive_scan(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned pre = 0u, sum = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) pre += s_w[w];
        sum += s_w[w];
    }
    __syncthreads();   // s_w may be written again by the caller's next round
    *total = sum;
    return pre + inc - v;
}

GS2M_KERNEL void __launch_bounds__(256)
k_bw_area_block_sums(GeomRecs recs, int P, unsigned* __restrict__ block_sum) {
    __shared__ unsigned s_w[4];
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    unsigned total;
    (void)bw_block_exclusive_scan(i < P ? bw_rect_area(recs.c[i]) : 0u, s_w, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one workgroup: block_sum[nb] -> its exclusive scan in place; *total_rows = the grand total (64-bit: checked by the host)
GS2M_KERNEL void __launch_bounds__(256)
k_bw_scan_blocks(unsigned* __restrict__ block_sum, int nb, unsigned long long* __restrict__ total_rows) {
    __shared__ unsigned s_w[4];
    unsigned long long carry = 0ull;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < nb ? block_sum[i] : 0u;
        unsigned total;
        const unsigned ex = bw_block_exclusive_scan(v, s_w, &total);
        if (i < nb) block_sum[i] = (unsigned)carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_rows = carry;
}

GS2M_KERNEL void __launch_bounds__(256)
k_bw_row_offsets(GeomRecs recs, int P, const unsigned* __restrict__ block_excl, unsigned* __restrict__ row_offset) {
    __shared__ unsigned s_w[4];
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    unsigned total;
    const unsigned ex = bw_block_exclusive_scan(i < P ? bw_rect_area(recs.c[i]) : 0u, s_w, &total);
    if (i < P) row_offset[i] = block_excl[blockIdx.x] + ex;
}

// SH basis values and their derivatives by the (unit) view direction, in the order of sh_channel (raster_math.h)
GS2M_DEVICE void bw_sh_basis(int deg, float x, float y, float z, float* b, float* bx, float* by, float* bz) {
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = bx[k] = by[k] = bz[k] = 0.0f;
    const float C1 = GS2M_SH_C1, c20 = 1.0925484305920792f, c22 = 0.31539156525252005f, c24 = 0.5462742152960396f;
    const float c30 = 0.5900435899266435f, c31 = 2.890611442640554f, c32 = 0.4570457994644658f, c33 = 0.3731763325901154f,
                c35 = 1.445305721320277f;
    b[0] = GS2M_SH_C0;
    if (deg < 1) return;
    b[1] = -C1 * y;
    by[1] = -C1;
    b[2] = C1 * z;
    bz[2] = C1;
    b[3] = -C1 * x;
    bx[3] = -C1;
    if (deg < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[4] = c20 * xy;
    bx[4] = c20 * y;
    by[4] = c20 * x;
    b[5] = -c20 * yz;
    by[5] = -c20 * z;
    bz[5] = -c20 * y;
    b[6] = c22 * (2.0f * zz - xx - yy);
    bx[6] = -2.0f * c22 * x;
    by[6] = -2.0f * c22 * y;
    bz[6] = 4.0f * c22 * z;
    b[7] = -c20 * xz;
    bx[7] = -c20 * z;
    bz[7] = -c20 * x;
    b[8] = c24 * (xx - yy);
    bx[8] = 2.0f * c24 * x;
    by[8] = -2.0f * c24 * y;
    if (deg < 3) return;
    b[9] = -c30 * y * (3.0f * xx - yy);
    bx[9] = -6.0f * c30 * xy;
    by[9] = -3.0f * c30 * (xx - yy);
    b[10] = c31 * xy * z;
    bx[10] = c31 * yz;
    by[10] = c31 * xz;
    bz[10] = c31 * xy;
    b[11] = -c32 * y * (4.0f * zz - xx - yy);
    bx[11] = 2.0f * c32 * xy;
    by[11] = -c32 * (4.0f * zz - xx - 3.0f * yy);
    bz[11] = -8.0f * c32 * yz;
    b[12] = c33 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    bx[12] = -6.0f * c33 * xz;
    by[12] = -6.0f * c33 * yz;
    bz[12] = 3.0f * c33 * (2.0f * zz - xx - yy);
    b[13] = -c32 * x * (4.0f * zz - xx - yy);
    bx[13] = -c32 * (4.0f * zz - 3.0f * xx - yy);
    by[13] = 2.0f * c32 * xy;
    bz[13] = -8.0f * c32 * xz;
    b[14] = c35 * z * (xx - yy);
    bx[14] = 2.0f * c35 * xz;
    by[14] = -2.0f * c35 * yz;
    bz[14] = c35 * (xx - yy);
    b[15] = -c30 * x * (xx - 3.0f * yy);
    bx[15] = -3.0f * c30 * (xx - yy);
    by[15] = 6.0f * c30 * xy;
}

// DEPTH: the rows carry dL/dz of the centre's view-space depth as their tenth value (gs2m_rasterize_backward_depth,
// raster_backward_blend.h); its sum times the view matrix's z row is added to dL/dmean3D.  DEPTH = false never reads that value.
template <bool DEPTH>
GS2M_KERNEL void __launch_bounds__(256)
k_gaussian_backward(GaussIn g, const CamUniform* __restrict__ cams, GeomRecs recs, const unsigned* __restrict__ row_offset,
                    const float* __restrict__ rows, unsigned long long n_rows, BwOut o) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.P) return;
    const CamUniform& cam = cams[0];
    const float* vm = cam.view;
    const float* pm = cam.proj;
    const float px = g.xyz[3 * (size_t)i], py = g.xyz[3 * (size_t)i + 1], pz = g.xyz[3 * (size_t)i + 2];
    float cov3[6];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, qr = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (g.cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) cov3[k] = g.cov3D_precomp[6 * (size_t)i + k];
    } else {
        sx = g.scales[3 * (size_t)i];
        sy = g.scales[3 * (size_t)i + 1];
        sz = g.scales[3 * (size_t)i + 2];
        qr = g.rots[4 * (size_t)i];
        qx = g.rots[4 * (size_t)i + 1];
        qy = g.rots[4 * (size_t)i + 2];
        qz = g.rots[4 * (size_t)i + 3];
        cov3d_from_scale_rot(sx, sy, sz, g.scale_modifier, qr, qx, qy, qz, cov3);
    }
    ProjView pv;
    project_view(cam, px, py, pz, cov3, pv);   // the forward's own visibility decision (radius > 0)
    const int ncoef = (g.D + 1) * (g.D + 1);
    float dmean[3] = {0.0f, 0.0f, 0.0f}, dcov[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float dscale[3] = {0.0f, 0.0f, 0.0f}, drot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
    float accz = 0.0f;
    if (pv.ok) {
        // ---- the Gaussian's instance rows, in slot order
        const unsigned n = bw_rect_area(recs.c[i]);
        const unsigned long long first = row_offset[i];
        for (unsigned s = 0; s < n && first + s < n_rows; ++s) {
            const float4* r4 = reinterpret_cast<const float4*>(rows + (size_t)(first + s) * GS2M_BW_ROW);
            const float4 a = r4[0], b = r4[1];
            const float c = r4[2].x;
            acc[0] += a.x;
            acc[1] += a.y;
            acc[2] += a.z;
            acc[3] += a.w;
            acc[4] += b.x;
            acc[5] += b.y;
            acc[6] += b.z;
            acc[7] += b.w;
            acc[8] += c;
            if constexpr (DEPTH) accz += r4[2].y;
        }
        // ---- conic -> cov2D -> cov3D and mean (backward.cu:144-274).  T = W J as in cov2d_ewa (raster_math.h): rows
        // T0 = (T00, T01, T02), T1 = (T10, T11, T12); a = T0 V T0^T + 0.3, b = T0 V T1^T, c = T1 V T1^T + 0.3
        float tvx, tvy, tvz;
        xform4x3(vm, px, py, pz, tvx, tvy, tvz);
        const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
        const float txtz = tvx / tvz, tytz = tvy / tvz;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * tvz, ty = fminf(limy, fmaxf(-limy, tytz)) * tvz;
        const float x_mul = (txtz < -limx || txtz > limx) ? 0.0f : 1.0f;   // backward.cu:175-176
        const float y_mul = (tytz < -limy || tytz > limy) ? 0.0f : 1.0f;
        const float fx = cam.focal_x, fy = cam.focal_y;
        const float J00 = fx / tvz, J02 = -(fx * tx) / (tvz * tvz), J11 = fy / tvz, J12 = -(fy * ty) / (tvz * tvz);
        const float T00 = vm[0] * J00 + vm[2] * J02, T01 = vm[4] * J00 + vm[6] * J02, T02 = vm[8] * J00 + vm[10] * J02;
        const float T10 = vm[1] * J11 + vm[2] * J12, T11 = vm[5] * J11 + vm[6] * J12, T12 = vm[9] * J11 + vm[10] * J12;
        // V T0^T and V T1^T
        const float U0 = cov3[0] * T00 + cov3[1] * T01 + cov3[2] * T02;
        const float U1 = cov3[1] * T00 + cov3[3] * T01 + cov3[4] * T02;
        const float U2 = cov3[2] * T00 + cov3[4] * T01 + cov3[5] * T02;
        const float Q0 = cov3[0] * T10 + cov3[1] * T11 + cov3[2] * T12;
        const float Q1 = cov3[1] * T10 + cov3[3] * T11 + cov3[4] * T12;
        const float Q2 = cov3[2] * T10 + cov3[4] * T11 + cov3[5] * T12;
        const float a = (T00 * U0 + T01 * U1 + T02 * U2) + 0.3f;
        const float b = T00 * Q0 + T01 * Q1 + T02 * Q2;
        const float c = (T10 * Q0 + T11 * Q1 + T12 * Q2) + 0.3f;
        const float det = a * c - b * b;
        const float d2i = 1.0f / (det * det + 0.0000001f);   // backward.cu:203
        const float gA = acc[2], gB = acc[3], gC = acc[4];
        // conic = (c, -b, a) / det
        const float da = d2i * (-c * c * gA + 2.0f * b * c * gB + (det - a * c) * gC);
        const float dc = d2i * (-a * a * gC + 2.0f * a * b * gB + (det - a * c) * gA);
        const float db = d2i * 2.0f * (b * c * gA - (det + 2.0f * b * b) * gB + a * b * gC);
        dcov[0] = T00 * T00 * da + T00 * T10 * db + T10 * T10 * dc;
        dcov[3] = T01 * T01 * da + T01 * T11 * db + T11 * T11 * dc;
        dcov[5] = T02 * T02 * da + T02 * T12 * db + T12 * T12 * dc;
        // off-diagonal entries of the symmetric Sigma appear twice
        dcov[1] = 2.0f * T00 * T01 * da + (T00 * T11 + T01 * T10) * db + 2.0f * T10 * T11 * dc;
        dcov[2] = 2.0f * T00 * T02 * da + (T00 * T12 + T02 * T10) * db + 2.0f * T10 * T12 * dc;
        dcov[4] = 2.0f * T02 * T01 * da + (T01 * T12 + T02 * T11) * db + 2.0f * T11 * T12 * dc;
        const float dT00 = 2.0f * U0 * da + Q0 * db, dT01 = 2.0f * U1 * da + Q1 * db, dT02 = 2.0f * U2 * da + Q2 * db;
        const float dT10 = 2.0f * Q0 * dc + U0 * db, dT11 = 2.0f * Q1 * dc + U1 * db, dT12 = 2.0f * Q2 * dc + U2 * db;
        const float dJ00 = vm[0] * dT00 + vm[4] * dT01 + vm[8] * dT02;
        const float dJ02 = vm[2] * dT00 + vm[6] * dT01 + vm[10] * dT02;
        const float dJ11 = vm[1] * dT10 + vm[5] * dT11 + vm[9] * dT12;
        const float dJ12 = vm[2] * dT10 + vm[6] * dT11 + vm[10] * dT12;
        const float iz = 1.0f / tvz, iz2 = iz * iz, iz3 = iz2 * iz;
        const float dtx = x_mul * -fx * iz2 * dJ02;
        const float dty = y_mul * -fy * iz2 * dJ12;
        const float dtz = -fx * iz2 * dJ00 - fy * iz2 * dJ11 + (2.0f * fx * tx) * iz3 * dJ02 + (2.0f * fy * ty) * iz3 * dJ12;
        dmean[0] = vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
        dmean[1] = vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
        dmean[2] = vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
        // ---- mean2D (NDC units) -> mean3D through the perspective division (backward.cu:372-387)
        {
            const float hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15];
            const float m_w = 1.0f / (hw + 0.0000001f);
            const float mul1 = (pm[0] * px + pm[4] * py + pm[8] * pz + pm[12]) * m_w * m_w;
            const float mul2 = (pm[1] * px + pm[5] * py + pm[9] * pz + pm[13]) * m_w * m_w;
            const float gx2 = acc[0], gy2 = acc[1];
            dmean[0] += (pm[0] * m_w - pm[3] * mul1) * gx2 + (pm[1] * m_w - pm[3] * mul2) * gy2;
            dmean[1] += (pm[4] * m_w - pm[7] * mul1) * gx2 + (pm[5] * m_w - pm[7] * mul2) * gy2;
            dmean[2] += (pm[8] * m_w - pm[11] * mul1) * gx2 + (pm[9] * m_w - pm[11] * mul2) * gy2;
        }
        if constexpr (DEPTH) {   // z = vm[2] x + vm[6] y + vm[10] z + vm[14] (the record's depth)
            dmean[0] += vm[2] * accz;
            dmean[1] += vm[6] * accz;
            dmean[2] += vm[10] * accz;
        }
    }
    // ---- colour -> SH coefficients and view direction (backward.cu:20-139)
    if (o.dL_dsh) {
        float* dsh = o.dL_dsh + (size_t)i * g.M * 3;
        if (pv.ok && g.shs) {
            const float* sh = g.shs + (size_t)i * g.M * 3;
            const float ox = px - cam.campos[0], oy = py - cam.campos[1], oz = pz - cam.campos[2];
            const float len = sqrtf(ox * ox + oy * oy + oz * oz);
            const float x = ox / len, y = oy / len, z = oz / len;
            // clamp flags from the colour the forward itself stored in the record (max(0, colour), whichever of its SH paths
            // computed it): a channel stored as 0 passes no gradient.  The reference flags colour < 0 only, so a colour of
            // EXACTLY 0 passes its gradient there and not here -- the one value where the two differ.
            const float4 rec_b = recs.ab[2 * (size_t)i + 1];
            const float rec_rgb[3] = {rec_b.z, rec_b.w, recs.c[i].x};
            float dRGB[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dRGB[c] = rec_rgb[c] > 0.0f ? acc[6 + c] : 0.0f;
            float bk[16], bx[16], by[16], bz[16];
            bw_sh_basis(g.D, x, y, z, bk, bx, by, bz);
            float ddir[3] = {0.0f, 0.0f, 0.0f};
            for (int k = 0; k < g.M; ++k) {
                const bool live = k < ncoef && k < 16;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dsh[3 * k + c] = live ? bk[k] * dRGB[c] : 0.0f;
                    if (live) {
                        const float s = sh[3 * k + c] * dRGB[c];
                        ddir[0] += bx[k] * s;
                        ddir[1] += by[k] * s;
                        ddir[2] += bz[k] * s;
                    }
                }
            }
            // through dir = v / |v|: (|v|^2 I - v v^T) / |v|^3
            const float sum2 = ox * ox + oy * oy + oz * oz;
            const float inv32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
            dmean[0] += ((sum2 - ox * ox) * ddir[0] - oy * ox * ddir[1] - oz * ox * ddir[2]) * inv32;
            dmean[1] += (-ox * oy * ddir[0] + (sum2 - oy * oy) * ddir[1] - oz * oy * ddir[2]) * inv32;
            dmean[2] += (-ox * oz * ddir[0] - oy * oz * ddir[1] + (sum2 - oz * oz) * ddir[2]) * inv32;
        } else {
            for (int k = 0; k < g.M * 3; ++k) dsh[k] = 0.0f;
        }
    }
    // ---- Sigma = A A^T, A = R diag(mod s) -> scale, rotation (backward.cu:278-341)
    if (pv.ok && !g.cov3D_precomp) {
        const float mod = g.scale_modifier;
        const float s0 = mod * sx, s1 = mod * sy, s2 = mod * sz;
        const float r = qr, x = qx, y = qy, z = qz;
        const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                               {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                               {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
        const float sv[3] = {s0, s1, s2};
        // symmetric dL/dSigma: the stored off-diagonal gradients count both entries
        const float G[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                               {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                               {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
        // dL/dA = 2 G A, A[i][j] = R[i][j] s_j;  dL/ds_j = sum_i dL/dA[i][j] R[i][j];  dL/dR[i][j] = dL/dA[i][j] s_j
        float dR[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float ds = 0.0f;
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) {
                const float dA = 2.0f * (G[ii][0] * R[0][j] + G[ii][1] * R[1][j] + G[ii][2] * R[2][j]) * sv[j];
                ds += dA * R[ii][j];
                dR[ii][j] = dA * sv[j];
            }
            dscale[j] = mod * ds;
        }
        // R(q) as written above, q used as given (no normalisation, backward.cu:281)
        drot[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
        drot[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1]) -
                  4.f * x * (dR[1][1] + dR[2][2]);
        drot[2] = 2.f * (x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1]) -
                  4.f * y * (dR[0][0] + dR[2][2]);
        drot[3] = 2.f * (-r * dR[0][1] + x * dR[0][2] + r * dR[1][0] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]) -
                  4.f * z * (dR[0][0] + dR[1][1]);
    }
    o.dL_dmean2D[3 * (size_t)i] = acc[0];
    o.dL_dmean2D[3 * (size_t)i + 1] = acc[1];
    o.dL_dmean2D[3 * (size_t)i + 2] = 0.0f;
    if (o.dL_dconic) {
        o.dL_dconic[4 * (size_t)i] = acc[2];
        o.dL_dconic[4 * (size_t)i + 1] = acc[3];
        o.dL_dconic[4 * (size_t)i + 2] = 0.0f;
        o.dL_dconic[4 * (size_t)i + 3] = acc[4];
    }
    o.dL_dopacity[i] = acc[5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.dL_dcolor[3 * (size_t)i + k] = acc[6 + k];
        o.dL_dmean3D[3 * (size_t)i + k] = dmean[k];
        o.dL_dscale[3 * (size_t)i + k] = dscale[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) o.dL_dcov3D[6 * (size_t)i + k] = dcov[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) o.dL_drot[4 * (size_t)i + k] = drot[k];
}

// Per-Gaussian half of the gradients through the RAY maps (gs2m_rasterize_backward_depth_ray; the derivative is stated in
// include/gs2mesh_amd.h).  Runs after k_gaussian_backward<true>, which has written every output row and has taken row[9] -- the
// fallback's and the clamps' dL/dz_c -- to dL/dmean3D; this kernel ADDS what the second rows hold to dL_dmean3D, dL_dscale and
// dL_drot of the Gaussians the forward listed.  One thread per Gaussian: it sums the second rows {A (3), Bm (6), dL/dsz} in slot
// order (bitwise reproducible), recomputes R, M, mu, g and sz with the operations of k_ray_records, and applies the chain
//     dL/dc_k = w_k . A;   dL/dw_k = c_k A - 2 Bm w_k + dL/dc_k mu;   dL/dmu = sum_k dL/dc_k w_k;
//     w_k = f_k M[:,k], f_k = g_k / gmax, differentiated THROUGH gmax = g_m:  dL/dg_k = dL/df_k / gmax for k != m and
//     dL/dg_m = -(sum_{k != m} f_k dL/df_k) / gmax.  t is invariant under a common scaling of all (w_k, c_k), so
//     sum_k f_k dL/df_k = 0 and holding gmax constant gives the same gradient in exact arithmetic; in fp32 it does not:
//     dL/df_m is what is left of two large sums that cancel, and with gmax held constant that remainder goes straight into
//     the two large scales of a flat Gaussian.  Through gmax it is never used (f_m = g_m / g_m does not depend on g_m);
//     g = (s1 s2, s0 s2, s0 s1);
//     sz = sqrt(sum_k (s_k M[2][k])^2): the derivative through the square root is taken as 0 where the sum is 0;
//     M = W R(q) -> dL/dR -> dL/dq with q as given;   mu = W x + t -> dL/dmean3D;   s = mod scales: dL/dscale keeps the factor mod.
// A Gaussian whose ten sums are all zero (no pixel took its depth from the quotient or a clamp) is left as it is: its outputs keep
// the bits of the alpha path.
GS2M_KERNEL void __launch_bounds__(256)
k_gaussian_backward_ray(GaussIn g, const CamUniform* __restrict__ cams, GeomRecs recs, const unsigned* __restrict__ row_offset,
                        const float* __restrict__ rows2, unsigned long long n_rows, BwOut o) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.P) return;
    const unsigned n = bw_rect_area(recs.c[i]);
    if (n == 0u) return;   // in no list: no rows
    float m[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = 0.0f;
    const unsigned long long first = row_offset[i];
    for (unsigned s = 0; s < n && first + s < n_rows; ++s) {
        const float4* r4 = reinterpret_cast<const float4*>(rows2 + (size_t)(first + s) * GS2M_BW_ROW);
        const float4 a = r4[0], b = r4[1];
        const float2 c = make_float2(r4[2].x, r4[2].y);
        m[0] += a.x;
        m[1] += a.y;
        m[2] += a.z;
        m[3] += a.w;
        m[4] += b.x;
        m[5] += b.y;
        m[6] += b.z;
        m[7] += b.w;
        m[8] += c.x;
        m[9] += c.y;
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < 10; ++k) any = any || m[k] != 0.0f;   // a NaN sum counts
    if (!any) return;
    const float* vm = cams[0].view;
    const float mod = g.scale_modifier;
    const float s[3] = {mod * g.scales[3 * (size_t)i], mod * g.scales[3 * (size_t)i + 1], mod * g.scales[3 * (size_t)i + 2]};
    const float r = g.rots[4 * (size_t)i], x = g.rots[4 * (size_t)i + 1], y = g.rots[4 * (size_t)i + 2], z = g.rots[4 * (size_t)i + 3];
    const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                           {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                           {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    float M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[a][k] = vm[a] * R[0][k] + vm[4 + a] * R[1][k] + vm[8 + a] * R[2][k];
    const float px = g.xyz[3 * (size_t)i], py = g.xyz[3 * (size_t)i + 1], pz = g.xyz[3 * (size_t)i + 2];
    const float mu[3] = {vm[0] * px + vm[4] * py + vm[8] * pz + vm[12], vm[1] * px + vm[5] * py + vm[9] * pz + vm[13],
                         vm[2] * px + vm[6] * py + vm[10] * pz + vm[14]};
    const float gk[3] = {s[1] * s[2], s[0] * s[2], s[0] * s[1]};
    const float gmax = fmaxf(gk[0], fmaxf(gk[1], gk[2]));
    const bool oriented = gmax > 0.0f && gmax <= 3.402823466e+38f;
    const float A[3] = {m[0], m[1], m[2]};
    // Bm, symmetric: xx xy x / xy yy y / x y 1
    const float Bm[3][3] = {{m[3], m[4], m[5]}, {m[4], m[6], m[7]}, {m[5], m[7], m[8]}};
    float dM[3][3], ds[3] = {0.0f, 0.0f, 0.0f}, dmu[3] = {0.0f, 0.0f, 0.0f}, dg[3] = {0.0f, 0.0f, 0.0f};
    const int kmax = (gk[0] >= gk[1] && gk[0] >= gk[2]) ? 0 : (gk[1] >= gk[2] ? 1 : 2);   // gmax = g[kmax]
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) dM[a][k] = 0.0f;
    if (oriented) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = gk[k] / gmax;
            const float w[3] = {f * M[0][k], f * M[1][k], f * M[2][k]};
            const float c = w[0] * mu[0] + w[1] * mu[1] + w[2] * mu[2];
            const float dc = w[0] * A[0] + w[1] * A[1] + w[2] * A[2];
            float df = 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float Bw = Bm[a][0] * w[0] + Bm[a][1] * w[1] + Bm[a][2] * w[2];
                const float dw = c * A[a] - 2.0f * Bw + dc * mu[a];
                dmu[a] += dc * w[a];
                dM[a][k] = f * dw;
                df += dw * M[a][k];
            }
            dg[k] = df;
        }
        // through gmax: f_kmax is 1 whatever g[kmax] is, and g[kmax] divides the other two
        float through = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) through += k == kmax ? 0.0f : (gk[k] / gmax) * dg[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) dg[k] = (k == kmax ? -through : dg[k]) / gmax;
        ds[0] = dg[1] * s[2] + dg[2] * s[1];
        ds[1] = dg[0] * s[2] + dg[2] * s[0];
        ds[2] = dg[0] * s[1] + dg[1] * s[0];
    }
    const float a0 = s[0] * M[2][0], a1 = s[1] * M[2][1], a2 = s[2] * M[2][2];
    const float var = a0 * a0 + a1 * a1 + a2 * a2;
    if (var > 0.0f) {   // sz = sqrt(var); at var == 0 the derivative through the square root is taken as 0
        const float ak[3] = {a0, a1, a2};
        const float k_sz = m[9] / sqrtf(var);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float da = k_sz * ak[k];
            ds[k] += da * M[2][k];
            dM[2][k] += da * s[k];
        }
    }
    // M = W R: dL/dR[b][k] = sum_a W[a][b] dL/dM[a][k], W[a][b] = vm[4 b + a]
    float dR[3][3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int k = 0; k < 3; ++k) dR[b][k] = vm[4 * b] * dM[0][k] + vm[4 * b + 1] * dM[1][k] + vm[4 * b + 2] * dM[2][k];
    float drot[4];
    drot[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
    drot[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1]) -
              4.f * x * (dR[1][1] + dR[2][2]);
    drot[2] = 2.f * (x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1]) -
              4.f * y * (dR[0][0] + dR[2][2]);
    drot[3] = 2.f * (-r * dR[0][1] + x * dR[0][2] + r * dR[1][0] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]) -
              4.f * z * (dR[0][0] + dR[1][1]);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        o.dL_dmean3D[3 * (size_t)i + b] += vm[4 * b] * dmu[0] + vm[4 * b + 1] * dmu[1] + vm[4 * b + 2] * dmu[2];
        o.dL_dscale[3 * (size_t)i + b] += mod * ds[b];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o.dL_drot[4 * (size_t)i + k] += drot[k];
}
