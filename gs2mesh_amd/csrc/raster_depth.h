// raster_depth.h -- depth and opacity maps of the last single-view forward (gs2m_rasterize_depth).
//
// The reference's renderCUDA writes colour only; these maps are an extension, stated here and in
// include/gs2mesh_amd.h.  The kernel is the shared front-to-back tile walk (raster_tile_walk.h: prologue, batch gather and step,
// the ones walk 1 of the compositing backward runs) with the three accumulators carried and the median's z recorded: one wave
// per 16 x 16 tile, four pixels per lane as the tile's four 8 x 8 quadrants, 64 instances of the tile's sorted list staged per
// batch into LDS, the three decisions of renderCUDA taken by bw_alpha on the staged record.
//
// Per pixel, T = 1, S = 0, Z = 0, med = 0; for every instance j of the tile's list, front to back (walk_step):
//     (ok, alpha) = bw_alpha(...)                      skip the instance if !ok
//     T' = T (1 - alpha); if T' < 1e-4 the pixel is finished -- BEFORE accumulating, as renderCUDA stops (forward.cu:345-350)
//     S = fma(T, alpha, S);  w = alpha T (rounded);  Z = fma(w, z_j, Z);  T = T'
//     if med == 0 and T <= 0.5: med = z_j              the first instance that takes the transmittance to one half or below
// and then   alpha = 1 - T,   depth_expected = S > 0 ? Z / S : 0,   depth_median = med.
// z_j is the view-space z of the Gaussian's CENTRE (recs.c[gid].y, the value the sort key carries), not the intersection of the
// pixel's ray with anything.  A pixel without a contributor holds exactly 0 in all three maps; z > 0.2 for every listed
// Gaussian (the near cull), so 0 means "no depth".  1 - T is exact for T in [0.5, 1]: depth_median > 0 exactly where alpha >= 0.5.
//
// Gradients through these maps: k_blend_backward<WPB, true> (raster_backward_blend.h), whose walk 1 is the same walk_step: its
// S, Z and median instance are this kernel's by construction.
//
// No atomics, plain stores: every pixel of the image is written exactly once by the lane that owns it, the pixels of tiles with
// an empty list included.
//
// RAY (gs2m_rasterize_depth_ray, raster_depth_ray.h): the same walk with z_j(p), the depth at which the pixel's ray meets the
// Gaussian, where z_j stands; the instance's 64-byte ray record is staged next to a, b and z.  Without RAY none of `ray`,
// `tanfovx` and `tanfovy` is read and the kernel is the one it was.
#pragma once
#include "raster_depth_ray.h"
#include "raster_tile_walk.h"

// grid: ceil(tiles / WPB) workgroups of WPB waves; wave w of workgroup b walks tile b * WPB + w.  Any output may be null.
template <int WPB, bool RAY = false>
GS2M_KERNEL void __launch_bounds__(64 * WPB)
k_blend_depth(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ tile_start, const GeomRecs recs, int P,
              unsigned cap, int W, int H, int gx, int gy, float* __restrict__ depth_expected, float* __restrict__ depth_median,
              float* __restrict__ alpha_out, const float4* __restrict__ ray, float tanfovx, float tanfovy) {
    // staged instance: a = {mx, my, ca, cb}, b = {cc, op, r, g}, z = view-space depth of the centre
    __shared__ float4 s_a[WPB][64], s_b[WPB][64];
    __shared__ float s_z[WPB][64];
    const int tile = walk_tile_of_wave<WPB>();
    if (tile >= gx * gy) return;
    const TileWalk t = walk_tile(tile, tile_start, cap, W, H, gx);
    float4* sa = &s_a[t.wave][0];
    float4* sb = &s_b[t.wave][0];
    float* sz = &s_z[t.wave][0];
    float T[4], S[4], Z[4], med[4];
    bool done[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        T[k] = 1.0f;
        S[k] = Z[k] = med[k] = 0.0f;
        done[k] = !t.inside[k];
    }
    float4* sr = nullptr;
    float rx[4], ry[4];
    if constexpr (RAY) {
        // vector v of instance j of wave w at s_r[w][v][j]: the staging lanes' 16-B stores are contiguous per vector
        __shared__ float4 s_r[WPB][GS2M_RAY_REC][64];
        sr = &s_r[t.wave][0][0];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rx[k] = ray_dir(t.pxf[k], W, tanfovx);
            ry[k] = ray_dir(t.pyf[k], H, tanfovy);
        }
    }
    // an empty list (r1 <= r0) runs no batch and falls through to the stores
    for (unsigned base = t.r0; base < t.r1; base += 64u) {
        if (gs2m_ballot_b(!(done[0] && done[1] && done[2] && done[3])) == 0ull) break;
        if constexpr (RAY) {
            // the hook gets the guarded id only: an id the forward cannot have written (walk_gather stages it with opacity 0)
            // stages a zero record, whatever record 0 holds
            walk_gather<true>(t, base, keys, recs, P, sa, sb, sz, [=](const unsigned gid, float4) {
                const bool known = (unsigned)(keys[base + t.lane] & 0xffffffffull) < (unsigned)P;
#pragma unroll
                for (int v = 0; v < GS2M_RAY_REC; ++v)
                    sr[64 * v + t.lane] = known ? ray[GS2M_RAY_REC * (size_t)gid + v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            });
        } else {
            walk_gather<true>(t, base, keys, recs, P, sa, sb, sz, [](unsigned, float4) {});
        }
        const int nb = (int)(t.r1 - base) < 64 ? (int)(t.r1 - base) : 64;
        for (int j = 0; j < nb; ++j) {
            const float4 A = sa[j], B = sb[j];
            const float z = sz[j];
            if constexpr (RAY) {
                const float4 w0 = sr[j], w1 = sr[64 + j], w2 = sr[128 + j], lim = sr[192 + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float zp = ray_depth(w0, w1, w2, lim, z, rx[k], ry[k]);
                    walk_step<true, false>(A, B, zp, t.pxf[k], t.pyf[k], T[k], done[k], S[k], Z[k], med[k], zp, nullptr, 0);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    walk_step<true, false>(A, B, z, t.pxf[k], t.pyf[k], T[k], done[k], S[k], Z[k], med[k], z, nullptr, 0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!t.inside[k]) continue;
        const size_t pix = (size_t)t.y[k] * W + t.x[k];
        if (alpha_out) alpha_out[pix] = 1.0f - T[k];
        if (depth_expected) depth_expected[pix] = S[k] > 0.0f ? Z[k] / S[k] : 0.0f;
        if (depth_median) depth_median[pix] = med[k];
    }
}
