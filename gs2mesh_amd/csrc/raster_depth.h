// raster_depth.h -- depth and opacity maps of the last single-view forward (gs2m_rasterize_depth).
//
// The reference's renderCUDA writes colour only; these maps are an extension, stated here and in
// include/gs2mesh_amd.h.  The kernel is walk 1 of the compositing backward (raster_backward_blend.h) with three accumulators: one
// wave per 16 x 16 tile, four pixels per lane as the tile's four 8 x 8 quadrants, 64 instances of the tile's sorted list staged
// per batch into LDS, the three decisions of renderCUDA taken by bw_alpha on the staged record.  It lives in the same unit as
// the backward, so bw_alpha rounds here as it does there.
//
// Per pixel, T = 1, S = 0, Z = 0, med = 0; for every instance j of the tile's list, front to back:
//     (ok, alpha) = bw_alpha(...)                      skip the instance if !ok
//     T' = T (1 - alpha); if T' < 1e-4 the pixel is finished -- BEFORE accumulating, as renderCUDA stops (forward.cu:345-350)
//     w = alpha T;  S += w;  Z += w z_j;  T = T'
//     if med == 0 and T <= 0.5: med = z_j              the first instance that takes the transmittance to one half or below
// and then   alpha = 1 - T,   depth_expected = S > 0 ? Z / S : 0,   depth_median = med.
// z_j is the view-space z of the Gaussian's CENTRE (recs.c[gid].y, the value the sort key carries), not the intersection of the
// pixel's ray with anything.  A pixel without a contributor holds exactly 0 in all three maps; z > 0.2 for every listed
// Gaussian (the near cull), so 0 means "no depth".  1 - T is exact for T in [0.5, 1]: depth_median > 0 exactly where alpha >= 0.5.
//
// Gradients through these maps: k_blend_backward<WPB, true> (raster_backward_blend.h), which repeats this walk's S and Z operation
// for operation.
//
// No atomics, plain stores: every pixel of the image is written exactly once by the lane that owns it, the pixels of tiles with
// an empty list included.
#pragma once
#include "raster_backward_blend.h"

// grid: ceil(tiles / WPB) workgroups of WPB waves; wave w of workgroup b walks tile b * WPB + w.  Any output may be null.
template <int WPB>
GS2M_KERNEL void __launch_bounds__(64 * WPB)
k_blend_depth(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ tile_start, const GeomRecs recs, int P,
              unsigned cap, int W, int H, int gx, int gy, float* __restrict__ depth_expected, float* __restrict__ depth_median,
              float* __restrict__ alpha_out) {
    // staged instance: a = {mx, my, ca, cb}, b = {cc, op, r, g}, z = view-space depth of the centre
    __shared__ float4 s_a[WPB][64], s_b[WPB][64];
    __shared__ float s_z[WPB][64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int tiles = gx * gy;
    const int tile = gs2m_uniform((int)blockIdx.x * WPB + wave);
    if (tile >= tiles) return;
    const int ty = tile / gx, tx = tile - ty * gx;
    float4* sa = &s_a[wave][0];
    float4* sb = &s_b[wave][0];
    float* sz = &s_z[wave][0];
    unsigned r0 = tile_start[tile], r1 = tile_start[tile + 1];
    if (r0 > cap) r0 = cap;
    if (r1 > cap) r1 = cap;
    r0 = (unsigned)gs2m_uniform((int)r0);
    r1 = (unsigned)gs2m_uniform((int)r1);
    const int px0 = tx * GS2M_TILE + (lane & 7), py0 = ty * GS2M_TILE + (lane >> 3);
    float pxf[4], pyf[4], T[4], S[4], Z[4], med[4];
    bool done[4], inside[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = px0 + 8 * (k & 1), y = py0 + 8 * (k >> 1);
        inside[k] = x < W && y < H;
        pxf[k] = (float)x;
        pyf[k] = (float)y;
        T[k] = 1.0f;
        S[k] = Z[k] = med[k] = 0.0f;
        done[k] = !inside[k];
    }
    // an empty list (r1 <= r0) runs no batch and falls through to the stores
    for (unsigned base = r0; base < r1; base += 64u) {
        if (gs2m_ballot_b(!(done[0] && done[1] && done[2] && done[3])) == 0ull) break;
        // the 64 instances [base, base + 64) of the list -> LDS (lane l stages instance base + l)
        gs2m_wave_sync();   // the previous batch has been read by every lane
        if (base + (unsigned)lane < r1) {
            unsigned gid = (unsigned)(keys[base + lane] & 0xffffffffull);
            const bool known = gid < (unsigned)P;   // never index the records with an id the forward cannot have written
            gid = known ? gid : 0u;
            sa[lane] = recs.ab[2 * (size_t)gid];
            float4 rb = recs.ab[2 * (size_t)gid + 1];
            if (!known) rb.y = 0.0f;   // opacity 0: alpha < 1/255 everywhere, the instance is skipped
            sb[lane] = rb;
            sz[lane] = known ? recs.c[gid].y : 0.0f;
        }
        gs2m_wave_sync();
        const int nb = (int)(r1 - base) < 64 ? (int)(r1 - base) : 64;
        for (int j = 0; j < nb; ++j) {
            const float4 A = sa[j], B = sb[j];
            const float z = sz[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float dx, dy, G, alpha;
                const bool ok = bw_alpha(A, B, pxf[k], pyf[k], dx, dy, G, alpha) && !done[k];
                const float test_T = T[k] * (1.0f - alpha);
                const bool sat = ok && test_T < 0.0001f;     // stop BEFORE accumulating (forward.cu:345-350)
                done[k] = done[k] || sat;
                if (ok && !sat) {
                    const float w = alpha * T[k];
                    S[k] += w;
                    Z[k] = fmaf(w, z, Z[k]);
                    T[k] = test_T;
                    if (med[k] == 0.0f && test_T <= 0.5f) med[k] = z;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!inside[k]) continue;
        const size_t pix = (size_t)(py0 + 8 * (k >> 1)) * W + (px0 + 8 * (k & 1));
        if (alpha_out) alpha_out[pix] = 1.0f - T[k];
        if (depth_expected) depth_expected[pix] = S[k] > 0.0f ? Z[k] / S[k] : 0.0f;
        if (depth_median) depth_median[pix] = med[k];
    }
}
