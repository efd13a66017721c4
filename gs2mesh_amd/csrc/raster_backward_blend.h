// raster_backward_blend.h -- backward of the per-tile compositing (the reference's backward renderCUDA, backward.cu:400-557).
//
// One wave per 16 x 16 tile, four pixels per lane laid out as the tile's four 8 x 8 quadrants (the decomposition of the forward's
// variant 4, raster_blend.h).  The forward does not write final_T / n_contrib (raster_blend.h:8), so the wave walks the tile's
// sorted list TWICE with one alpha function (bw_alpha):
//   1. front to back: per pixel the transmittance after its last contributor (T_final) and the list position after that
//      contributor (n_contrib) -- the three decisions of renderCUDA, including stop-before-accumulate.  This is the shared
//      tile walk (raster_tile_walk.h: walk_tile, walk_gather, walk_step), the one k_blend_depth runs;
//   2. back to front from the wave's largest n_contrib: T is rebuilt by division (T / (1 - alpha), backward.cu:503), the colour
//      behind a contributor is carried as the reference's accum_rec recurrence (:515), and every contributing pixel adds to the
//      nine per-instance values  dL/dmean2D (2)  dL/dconic (3)  dL/dopacity (1)  dL/dcolour (3).
// Both walks evaluate bw_alpha on the same staged record with explicit FMAs, so they take the same threshold decisions.
//
// Accumulation across tiles WITHOUT float atomics (DESIGN.md "Backward accumulation"): the reference adds every pixel's
// contribution with atomicAdd (:523-554) -- 64 lanes into 64 different rows, the slowest shape global float atomics have on
// this chip, and a sum whose rounding depends on arrival order.  Here a lane first adds its four pixels, the wave reduces the nine
// values over its 64 lanes in registers (a transposing butterfly: 10 shuffles for eight of them, 6 for the ninth) and lanes 0..8
// store ONE row of GS2M_BW_ROW floats per (Gaussian, tile) instance with plain stores, at
//     row = offset[g] + (ty - y0) * (x1 - x0) + (tx - x0)       (the tile's slot inside the Gaussian's tile rect),
// so the rows of a Gaussian are contiguous and the per-Gaussian pass (raster_backward_project.h) sums them in slot order: the
// gradients are bitwise reproducible.  The reduction is skipped when no lane contributed; rows that are never written (instances
// behind every pixel's last contributor, tiles an exact cull level removed from the rect) read as zero because the row buffer is
// cleared before the launch.
//
// Departures of the reference's backward from the true derivative, reproduced here (they are the contract):
//   * min(0.99, o G) is ignored in the derivative -- straight-through (backward.cu:499, :541): dL/dG = o dL/dalpha and
//     dL/do = G dL/dalpha also where the cap binds;
//   * dL/dmean2D is accumulated in NDC-scaled units, 0.5 W and 0.5 H (:460-461);
//   * the background term  -T_final / (1 - alpha) * (bg . dL/dpixel)  (:531-534).
//
// Gradients through the depth and opacity maps (k_blend_backward<WPB, true>, gs2m_rasterize_backward_depth; an extension like
// the maps themselves).  Per pixel the forward walk of raster_depth.h gives, over the contributors j,  w_j = alpha_j T_j,
// S = sum w_j,  Z = sum w_j z_j,  T_f,  D = S > 0 ? Z / S : 0,  A = 1 - T_f  and  med = z_m, m the first contributor after
// which T <= 0.5.  With upstream gradients gD, gM, gA ([H,W] each, a null map = zeros):
//   * expected depth: one more "colour channel" over a zero background whose per-instance value is u_j = (gD / S)(z_j - D)
//     (0 where S == 0); it adds T_j (u_j - rec_j) to dL/dalpha_j, rec the same behind-the-contributor recurrence as colour's;
//   * opacity map: dA/dalpha_j = T_f / (1 - alpha_j), the shape of the background term: bgdot becomes bgdot - gA;
//   * dL/dz_j, the tenth value of the instance row (row[9]): every contributing pixel adds w_j gD / S, the pixel whose median
//     is this instance also adds gM.  med is piecewise constant in everything but z_m; that is the stated derivative.  The
//     per-Gaussian pass adds (vm[2], vm[6], vm[10]) sum(row[9]) to dL/dmean3D: z_j is the view-space z of the centre.
// dL/dalpha continues into mean2D, conic and opacity exactly as for colour, under the same departures.  Walk 1 is k_blend_depth's
// own walk_step with S and Z carried (S = fma(T, alpha, S); w = alpha T rounded; Z = fma(w, z, Z)) and the median's list position
// recorded where the depth pass records its z, so D has the forward's bits and the median is the forward's instance.  Values
// nine and ten share one 2-value butterfly (bw_reduce2).  The DEPTH = false instantiation is the colour backward unchanged: its
// walk_step carries no S, Z or median, and it neither reads nor writes row[9].
//
// Gradients through the RAY maps (k_blend_backward<WPB, true, true>, gs2m_rasterize_backward_depth_ray; the derivative is stated in
// include/gs2mesh_amd.h).  The depth of instance j at pixel p is z_j(p) = ray_depth() of the staged ray record
// (raster_depth_ray.h), brought to LDS by walk_gather's `extra` hook as k_blend_depth<WPB, true> does, so walk 1's D and median
// instance have the bits of gs2m_rasterize_depth_ray and u_j = (gD / S)(z_j(p) - D).  h = dL/dz_j(p), the amount the centre
// instantiation adds to row[9], goes where ray_depth() took z_j(p) from (ray_branch() repeats its decisions on its bits):
//   * t = num / den, lo <= t <= hi: ten moments  A += (h / den) r,  Bm += (h t / den) r r^T  (r = (rx, ry, 1); Bm in the order
//     xx, xy, x, yy, y, 1) -- dt/dc_k = u_k / den and dt/dw_k = ((c_k - 2 t u_k) / den) r summed over the pixels;
//   * the fallback t = z_c, and a clamp at hi or at lo = z_c - 4 sz: h to row[9]; the clamps also add +-4 h to dL/dsz;
//   * a clamp at the 0.2 floor: nothing.
// The eleven values are the instance's SECOND row, at rows2 + row * GS2M_BW_ROW: {A (3), Bm (6), dL/dsz, 0, 0}, reduced with one
// more bw_reduce8, one bw_reduce2 (Bm's last value and dL/dsz) and stored by lanes 0..9 as the first row is.  Written by the plain stores of
// the wave that wrote the first row, in an arena only this entry allocates and clears.  Without RAY nothing of this exists: the
// two other instantiations are the kernels they were.
#pragma once
#include "raster_depth_ray.h"
#include "raster_tile_walk.h"

// where ray_depth() took z_j(p) from: 0 the quotient t (lo <= t <= hi), 1 the fallback z_c, 2 the clamp at hi, 3 the clamp at
// lo = z_c - 4 sz, 4 the clamp at the 0.2 floor.  Same operations as ray_depth(), so the same bits decide; *t_out and *den_out are
// its quotient and denominator (read for branch 0 only).
GS2M_DEVICE int ray_branch(const float4 w0, const float4 w1, const float4 w2, const float4 lim, const float zc, const float rx,
                           const float ry, float* t_out, float* den_out) {
    const float u0 = fmaf(w0.x, rx, fmaf(w0.y, ry, w0.z));
    const float u1 = fmaf(w1.x, rx, fmaf(w1.y, ry, w1.z));
    const float u2 = fmaf(w2.x, rx, fmaf(w2.y, ry, w2.z));
    const float num = fmaf(w0.w, u0, fmaf(w1.w, u1, w2.w * u2));
    const float den = fmaf(u0, u0, fmaf(u1, u1, u2 * u2));
    const float q = num / den;
    const bool quotient = den > 0.0f && fabsf(q) <= 3.402823466e+38f;
    const float t = quotient ? q : zc;
    *t_out = t;
    *den_out = den;
    if (t > lim.y) return 2;
    if (t < lim.x) return lim.x > 0.2f ? 3 : 4;   // lo = max(z_c - 4 sz, 0.2): above the floor it is z_c - 4 sz
    return quotient ? 0 : 1;
}

// sum over the 64 lanes of eight per-lane values: afterwards lane l holds the complete sum of value 4 (l & 1) + 2 ((l >> 1) & 1) +
// ((l >> 2) & 1).  Each step halves the values a lane carries (it keeps one half, sends the other to its partner): 4 + 2 + 1
// shuffles, then 3 for the remaining lane bits.  The order of the additions is fixed by the lane number.
GS2M_DEVICE float bw_reduce8(const float* a, const int lane) {
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    float b[4], c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float recv = gs2m_shfl_xor(b0 ? a[k] : a[k + 4], 1);
        b[k] = (b0 ? a[k + 4] : a[k]) + recv;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float recv = gs2m_shfl_xor(b1 ? b[k] : b[k + 2], 2);
        c[k] = (b1 ? b[k + 2] : b[k]) + recv;
    }
    float d = (b2 ? c[1] : c[0]) + gs2m_shfl_xor(b2 ? c[0] : c[1], 4);
    d += gs2m_shfl_xor(d, 8);
    d += gs2m_shfl_xor(d, 16);
    d += gs2m_shfl_xor(d, 32);
    return d;
}
GS2M_DEVICE float bw_reduce1(float d) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) d += gs2m_shfl_xor(d, m);
    return d;
}

// sum over the 64 lanes of two per-lane values: afterwards every even lane holds the complete sum of a0 and every odd lane that
// of a1 (1 + 5 shuffles).  Floating-point addition commutes, so the sum of a0 has the bits bw_reduce1(a0) gives.
GS2M_DEVICE float bw_reduce2(const float a0, const float a1, const int lane) {
    const bool b0 = lane & 1;
    float d = (b0 ? a1 : a0) + gs2m_shfl_xor(b0 ? a0 : a1, 1);
#pragma unroll
    for (int m = 2; m < 64; m <<= 1) d += gs2m_shfl_xor(d, m);
    return d;
}

// upstream gradients of the depth and opacity maps (raster_depth.h), [H,W] each; a null map is a map of zeros
struct BwDepthGrads {
    const float* dL_ddepth;    // expected depth D = Z / S
    const float* dL_dmedian;   // median depth
    const float* dL_dalpha;    // accumulated opacity A = 1 - T_final
};

// grid: ceil(tiles / WPB) workgroups of WPB waves; wave w of workgroup b composites tile b * WPB + w of the (single) view.
// DEPTH = false is the colour backward (gs2m_rasterize_backward): dg is not read and row value 9 is not written.
// RAY (with DEPTH): z_j(p) is the ray-Gaussian intersection depth; `ray` = the records of k_ray_records, `rows2` = the second rows
template <int WPB, bool DEPTH, bool RAY = false>
GS2M_KERNEL void __launch_bounds__(64 * WPB)
k_blend_backward(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ tile_start, const GeomRecs recs,
                 const CamUniform* __restrict__ cams, int P, unsigned cap, const float* __restrict__ dL_dpix,
                 const unsigned* __restrict__ row_offset, float* __restrict__ rows, unsigned long long n_rows,
                 const BwDepthGrads dg, const float4* __restrict__ ray = nullptr, float* __restrict__ rows2 = nullptr) {
    static_assert(DEPTH || !RAY, "the ray instantiation is a depth instantiation");
    // staged instance: a = {mx, my, ca, cb}, b = {cc, op, r, g}, c = {b, row index (bits)}; DEPTH: z = view-space depth
    __shared__ float4 s_a[WPB][64], s_b[WPB][64];
    __shared__ float2 s_c[WPB][64];
    __shared__ float s_z[DEPTH ? WPB : 1][64];
    const CamUniform& cam = cams[0];
    const int W = cam.W, H = cam.H;
    const int tile = walk_tile_of_wave<WPB>();
    if (tile >= cam.gx * cam.gy) return;
    const TileWalk t = walk_tile(tile, tile_start, cap, W, H, cam.gx);
    const int lane = t.lane;
    const unsigned r0 = t.r0, r1 = t.r1;
    if (r1 <= r0) return;
    float4* sa = &s_a[t.wave][0];
    float4* sb = &s_b[t.wave][0];
    float2* sc = &s_c[t.wave][0];
    float* sz = &s_z[DEPTH ? t.wave : 0][0];
    const size_t plane = (size_t)H * W;
    float T[4], dp0[4], dp1[4], dp2[4];
    int ncontrib[4];     // list position (relative to r0) after the pixel's last contributor
    bool done[4];
    // DEPTH: walk 1 carries S, Z and the list position after the median contributor (0: none); walk 2 keeps gD / S in sS and
    // D in sZ
    float sS[4], sZ[4], gM[4];
    int medpos[4];
    float4* sr = nullptr;
    float rx[4], ry[4];
    if constexpr (RAY) {
        // vector v of instance j of wave w at s_r[w][v][j], as k_blend_depth<WPB, true> stages it
        __shared__ float4 s_r[WPB][GS2M_RAY_REC][64];
        sr = &s_r[t.wave][0][0];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rx[k] = ray_dir(t.pxf[k], W, cam.tanfovx);
            ry[k] = ray_dir(t.pyf[k], H, cam.tanfovy);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool inside = t.inside[k];
        T[k] = 1.0f;
        ncontrib[k] = 0;
        done[k] = !inside;
        const size_t pix = (size_t)t.y[k] * W + t.x[k];
        if constexpr (DEPTH) {
            const bool col = inside && dL_dpix != nullptr;
            dp0[k] = col ? dL_dpix[pix] : 0.0f;
            dp1[k] = col ? dL_dpix[plane + pix] : 0.0f;
            dp2[k] = col ? dL_dpix[2 * plane + pix] : 0.0f;
            sS[k] = sZ[k] = 0.0f;
            medpos[k] = 0;
        } else {
            dp0[k] = inside ? dL_dpix[pix] : 0.0f;
            dp1[k] = inside ? dL_dpix[plane + pix] : 0.0f;
            dp2[k] = inside ? dL_dpix[2 * plane + pix] : 0.0f;
        }
    }
    // the shared gather, extended by what walk 2 needs of an instance: its blue channel and its row
    auto stage = [&](const unsigned base) __attribute__((always_inline)) {
        walk_gather<DEPTH>(t, base, keys, recs, P, sa, sb, sz, [&](const unsigned gid, const float4 rc) __attribute__((always_inline)) {
            const unsigned rect0 = __float_as_uint(rc.z), rect1 = __float_as_uint(rc.w);
            const int x0 = (int)(rect0 & 0xffffu), y0 = (int)(rect0 >> 16), x1 = (int)(rect1 & 0xffffu);
            // slot of this tile inside the Gaussian's tile rect (the lists only hold tiles of the rect)
            const unsigned row = row_offset[gid] + (unsigned)((t.ty - y0) * (x1 - x0) + (t.tx - x0));
            float2 c;
            c.x = rc.x;
            c.y = __uint_as_float(row);
            sc[lane] = c;
            if constexpr (RAY) {   // an id the forward cannot have written stages a zero record (raster_depth.h)
                const bool known = (unsigned)(keys[base + lane] & 0xffffffffull) < (unsigned)P;
#pragma unroll
                for (int v = 0; v < GS2M_RAY_REC; ++v)
                    sr[64 * v + lane] = known ? ray[GS2M_RAY_REC * (size_t)gid + v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        });
    };
    // ---- walk 1, front to back: T_final and n_contrib of every pixel (forward.cu:324-357)
    for (unsigned base = r0; base < r1; base += 64u) {
        if (gs2m_ballot_b(!(done[0] && done[1] && done[2] && done[3])) == 0ull) break;
        stage(base);
        const int nb = (int)(r1 - base) < 64 ? (int)(r1 - base) : 64;
        for (int j = 0; j < nb; ++j) {
            const float4 A = sa[j], B = sb[j];
            float z = 0.0f;
            if constexpr (DEPTH) z = sz[j];
            const int pos = (int)(base - r0) + j + 1;
            if constexpr (RAY) {
                const float4 w0 = sr[j], w1 = sr[64 + j], w2 = sr[128 + j], lim = sr[192 + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float zp = ray_depth(w0, w1, w2, lim, z, rx[k], ry[k]);
                    walk_step<true, true>(A, B, zp, t.pxf[k], t.pyf[k], T[k], done[k], sS[k], sZ[k], medpos[k], pos, &ncontrib[k], pos);
                }
                continue;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)   // DEPTH = false: sS, sZ and medpos are not initialised, and walk_step does not touch them
                walk_step<DEPTH, true>(A, B, z, t.pxf[k], t.pyf[k], T[k], done[k], sS[k], sZ[k], medpos[k], pos, &ncontrib[k], pos);
        }
    }
    int nmax = ncontrib[0] > ncontrib[1] ? ncontrib[0] : ncontrib[1];
    nmax = nmax > ncontrib[2] ? nmax : ncontrib[2];
    nmax = nmax > ncontrib[3] ? nmax : ncontrib[3];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = gs2m_shfl_xor(nmax, m);
        nmax = o > nmax ? o : nmax;
    }
    nmax = gs2m_uniform(nmax);
    if (nmax == 0) return;
    // ---- walk 2, back to front (backward.cu:464-556)
    float Tf[4], bgdot[4], last_alpha[4], lc0[4], lc1[4], lc2[4], ar0[4], ar1[4], ar2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Tf[k] = T[k];
        bgdot[k] = cam.bg[0] * dp0[k] + cam.bg[1] * dp1[k] + cam.bg[2] * dp2[k];
        last_alpha[k] = 0.0f;
        lc0[k] = lc1[k] = lc2[k] = 0.0f;
        ar0[k] = ar1[k] = ar2[k] = 0.0f;
    }
    // DEPTH: the expected depth is one more channel of value u_j = (gD / S) (z_j - D) over a zero background, the opacity map
    // has the background term's shape:  dA/dalpha_j = T_final / (1 - alpha_j)
    float lu[4], aru[4];
    if constexpr (DEPTH) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // a pixel with a contributor lies inside the image and has S > 0 (alpha >= 1/255, T >= 1e-4); the others add nothing
            const bool live = ncontrib[k] > 0;
            const size_t pix = (size_t)t.y[k] * W + (size_t)t.x[k];
            const float S = sS[k];
            const float gD = (live && dg.dL_ddepth) ? dg.dL_ddepth[pix] : 0.0f;
            gM[k] = (live && dg.dL_dmedian) ? dg.dL_dmedian[pix] : 0.0f;
            const float gA = (live && dg.dL_dalpha) ? dg.dL_dalpha[pix] : 0.0f;
            sZ[k] = S > 0.0f ? sZ[k] / S : 0.0f;
            sS[k] = S > 0.0f ? gD / S : 0.0f;
            bgdot[k] -= gA;
            lu[k] = aru[k] = 0.0f;
        }
    }
    const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;   // pixel per NDC unit (backward.cu:460-461)
    for (int bi = (nmax - 1) / 64; bi >= 0; --bi) {
        const unsigned base = r0 + 64u * (unsigned)bi;
        stage(base);
        const int jtop = (nmax - 1 - 64 * bi) < 63 ? (nmax - 1 - 64 * bi) : 63;
        for (int j = jtop; j >= 0; --j) {
            const int idx = 64 * bi + j;
            const float4 A = sa[j], B = sb[j];
            const float2 Cc = sc[j];
            float acc[8], acc8 = 0.0f, acc9 = 0.0f;   // mx my ca cb cc op r g | b | z (DEPTH)
            float z = 0.0f;
            if constexpr (DEPTH) z = sz[j];
            // RAY: the second row {A (3), Bm xx xy x yy y} | {Bm 1, dL/dsz}
            float mo[8], mo8 = 0.0f, dsz = 0.0f;
            float4 w0, w1, w2, lim;
            if constexpr (RAY) {
                w0 = sr[j];
                w1 = sr[64 + j];
                w2 = sr[128 + j];
                lim = sr[192 + j];
#pragma unroll
                for (int i = 0; i < 8; ++i) mo[i] = 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float dx, dy, G, alpha;
                const bool ok = bw_alpha(A, B, t.pxf[k], t.pyf[k], dx, dy, G, alpha) && idx < ncontrib[k];
                if (ok) {
                    any = true;
                    T[k] = T[k] / (1.0f - alpha);
                    const float w = alpha * T[k];
                    // colour composited behind this contributor (the reference's accum_rec recurrence, backward.cu:515)
                    ar0[k] = last_alpha[k] * lc0[k] + (1.0f - last_alpha[k]) * ar0[k];
                    ar1[k] = last_alpha[k] * lc1[k] + (1.0f - last_alpha[k]) * ar1[k];
                    ar2[k] = last_alpha[k] * lc2[k] + (1.0f - last_alpha[k]) * ar2[k];
                    lc0[k] = B.z;
                    lc1[k] = B.w;
                    lc2[k] = Cc.x;
                    float dL_dalpha = (B.z - ar0[k]) * dp0[k] + (B.w - ar1[k]) * dp1[k] + (Cc.x - ar2[k]) * dp2[k];
                    if constexpr (RAY) {
                        const float zp = ray_depth(w0, w1, w2, lim, z, rx[k], ry[k]);
                        const float u = sS[k] * (zp - sZ[k]);
                        aru[k] = last_alpha[k] * lu[k] + (1.0f - last_alpha[k]) * aru[k];
                        lu[k] = u;
                        dL_dalpha += u - aru[k];
                        const float h = w * sS[k] + (idx + 1 == medpos[k] ? gM[k] : 0.0f);
                        float tq, den;
                        const int br = ray_branch(w0, w1, w2, lim, z, rx[k], ry[k], &tq, &den);
                        if (br == 0) {
                            const float hd = h / den, ht = hd * tq;
                            mo[0] += hd * rx[k];
                            mo[1] += hd * ry[k];
                            mo[2] += hd;
                            mo[3] += ht * rx[k] * rx[k];
                            mo[4] += ht * rx[k] * ry[k];
                            mo[5] += ht * rx[k];
                            mo[6] += ht * ry[k] * ry[k];
                            mo[7] += ht * ry[k];
                            mo8 += ht;
                        } else if (br != 4) {
                            acc9 += h;
                            dsz += br == 2 ? 4.0f * h : (br == 3 ? -4.0f * h : 0.0f);
                        }
                    } else if constexpr (DEPTH) {
                        const float u = sS[k] * (z - sZ[k]);
                        aru[k] = last_alpha[k] * lu[k] + (1.0f - last_alpha[k]) * aru[k];
                        lu[k] = u;
                        dL_dalpha += u - aru[k];
                        acc9 += w * sS[k] + (idx + 1 == medpos[k] ? gM[k] : 0.0f);
                    }
                    dL_dalpha *= T[k];
                    last_alpha[k] = alpha;
                    dL_dalpha += (-Tf[k] / (1.0f - alpha)) * bgdot[k];   // background term (backward.cu:531-534)
                    const float dL_dG = B.y * dL_dalpha;                // straight through the 0.99 cap (:499, :541)
                    const float gdx = G * dx, gdy = G * dy;
                    acc[0] += dL_dG * (-gdx * A.z - gdy * A.w) * ddelx_dx;
                    acc[1] += dL_dG * (-gdy * B.x - gdx * A.w) * ddely_dy;
                    acc[2] += -0.5f * gdx * dx * dL_dG;
                    acc[3] += -0.5f * gdx * dy * dL_dG;
                    acc[4] += -0.5f * gdy * dy * dL_dG;
                    acc[5] += G * dL_dalpha;
                    acc[6] += w * dp0[k];
                    acc[7] += w * dp1[k];
                    acc8 += w * dp2[k];
                }
            }
            if (gs2m_ballot_b(any) == 0ull) continue;   // no lane contributed: the row keeps its zeros
            const float s = bw_reduce8(acc, lane);
            float s8;
            if constexpr (DEPTH) s8 = bw_reduce2(acc8, acc9, lane);
            else s8 = bw_reduce1(acc8);
            const unsigned long long row = (unsigned long long)__float_as_uint(Cc.y);
            if (row < n_rows) {
                float* dst = rows + (size_t)row * GS2M_BW_ROW;
                // lane l < 8 holds value 4 (l & 1) + 2 ((l >> 1) & 1) + ((l >> 2) & 1); lane 8 stores the ninth
                if (lane < 8) dst[4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1)] = s;
                else if (lane == 8 || (DEPTH && lane == 9)) dst[lane] = s8;   // lane 9 (odd) holds the tenth value
            }
            if constexpr (RAY) {
                const float m = bw_reduce8(mo, lane);
                const float m8 = bw_reduce2(mo8, dsz, lane);   // even lanes: Bm's last value; odd lanes: dL/dsz
                if (row < n_rows) {
                    float* dst = rows2 + (size_t)row * GS2M_BW_ROW;
                    if (lane < 8) dst[4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1)] = m;
                    else if (lane == 8 || lane == 9) dst[lane] = m8;
                }
            }
        }
    }
}
