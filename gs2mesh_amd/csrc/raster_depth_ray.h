// raster_depth_ray.h -- ray-Gaussian intersection depth of the last single-view forward (gs2m_rasterize_depth_ray).
//
// raster_depth.h gives every contributor the view-space z of its CENTRE; on a surface that is not fronto-parallel that is a
// staircase.  Here the depth of instance j at pixel p is the view-space depth t at which the Gaussian's density is largest
// along the pixel's ray x = t r (r_z = 1):  t* = (r^T B mu) / (r^T B r),  B any positive multiple of adj(Sigma_view).  The
// adjugate exists for a singular Sigma: a disc of zero thickness gives the ray-plane intersection (n . mu) / (n . r).  The
// statement is in include/gs2mesh_amd.h; this file is its two kernels.
//
// 1. k_ray_records: one lane per Gaussian whose record of the forward has a non-empty tile rect (no walk reads another), from the
//    forward's inputs.  With W the view rotation (W[i][j] = viewmatrix[4 j + i], what computeCov2D reads), R(q) the rotation of
//    computeCov3D (q used as given), M = W R, s = scale_modifier * scales, mu the view-space mean (transformPoint4x3):
//        g = (s1 s2, s0 s2, s0 s1);  gmax = max g_k
//        if !(gmax > 0) or gmax not finite:  w_k = 0, c_k = 0        (rank <= 1: no orientation)
//        else  w_k = (g_k / gmax) * (column k of M),  c_k = w_k . mu
//        sz = sqrt(max(sum_k s_k^2 M[2][k]^2, 0))   lo = max(z_c - 4 sz, 0.2)   hi = z_c + 4 sz   (z_c = recs.c[gid].y)
//    so that B = sum_k w_k w_k^T: the factor form has no cancellation between terms and no 2 x 2 minors.  Contraction is off in
//    this kernel: every product and sum is rounded on its own, left to right, as the CPU build of the tests does.
//    The 64-byte record is {w0, c0} {w1, c1} {w2, c2} {lo, hi, 0, 0}: four 16-B vectors, written with plain stores.
//
// 2. k_blend_depth<WPB, true> (raster_depth.h): the walk of the centre maps, unchanged -- walk_tile, walk_gather, walk_step and
//    bw_alpha are shared with the backward pass and not edited -- with the record of every staged instance brought to LDS by
//    walk_gather's `extra` hook (an id the forward cannot have written stages zeros) and, per (instance, pixel), ray_depth():
//        r   = (((2 px + 1) / W - 1) tanfovx, ((2 py + 1) / H - 1) tanfovy, 1)        the inverse of ndc2Pix
//        u_k = fma(w_k.x, r.x, fma(w_k.y, r.y, w_k.z))
//        num = fma(c_0, u_0, fma(c_1, u_1, c_2 u_2));  den = fma(u_0, u_0, fma(u_1, u_1, u_2 u_2))
//        t   = (den > 0 and num / den finite) ? num / den : z_c;   z_j(p) = min(max(t, lo), hi)
//    standing where z_j stood: Z = fma(w, z_j(p), Z), and the median is z_j(p) of the first contributor that takes T to 0.5 or
//    below.  Explicit FMAs and an IEEE division: no choice is the compiler's.  The clamp is exact for every ray within 4 sigma of
//    the centre (the maximum along such a ray lies inside that ellipsoid) and bounds what an edge-on disc, visible only through
//    the 0.3 px dilation, can contribute.  Every z_j(p) is finite and in [lo, hi] within [0.2, inf) for a finite z_c: 0 still
//    means "no depth", and alpha does not depend on z at all (it has the bits of gs2m_rasterize_depth's).
//
// LDS: 4 KB more per wave (64 instances x 64 B), 25 KB per workgroup of four waves: six workgroups = 24 waves per CU
// (profiles/raster_depth_ray.txt).
#pragma once
#include "raster_tile_walk.h"

#define GS2M_RAY_REC 4   // float4 per ray record

// grid: ceil(P / 256) workgroups of 256 lanes, lane = Gaussian
GS2M_KERNEL void __launch_bounds__(256)
k_ray_records(const GeomRecs recs, const int P, const float* __restrict__ means3D, const float* __restrict__ scales,
              const float mod, const float* __restrict__ rots, const float* __restrict__ vm, float4* __restrict__ ray) {
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    const float4 rc = recs.c[i];
    const unsigned rect0 = __float_as_uint(rc.z), rect1 = __float_as_uint(rc.w);
    if (!((rect1 & 0xffffu) > (rect0 & 0xffffu) && (rect1 >> 16) > (rect0 >> 16))) return;   // in no list
    const float s[3] = {mod * scales[3 * (size_t)i], mod * scales[3 * (size_t)i + 1], mod * scales[3 * (size_t)i + 2]};
    const float r = rots[4 * (size_t)i], x = rots[4 * (size_t)i + 1], y = rots[4 * (size_t)i + 2], z = rots[4 * (size_t)i + 3];
    // forward.cu:118-152 computeCov3D's R, row by row
    const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                           {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                           {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    float M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[a][k] = vm[a] * R[0][k] + vm[4 + a] * R[1][k] + vm[8 + a] * R[2][k];
    const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
    const float mu[3] = {vm[0] * px + vm[4] * py + vm[8] * pz + vm[12], vm[1] * px + vm[5] * py + vm[9] * pz + vm[13],
                         vm[2] * px + vm[6] * py + vm[10] * pz + vm[14]};
    const float g[3] = {s[1] * s[2], s[0] * s[2], s[0] * s[1]};
    const float gmax = fmaxf(g[0], fmaxf(g[1], g[2]));
    const bool oriented = gmax > 0.0f && gmax <= 3.402823466e+38f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (oriented) {
            const float f = g[k] / gmax;
            o.x = f * M[0][k];
            o.y = f * M[1][k];
            o.z = f * M[2][k];
            o.w = o.x * mu[0] + o.y * mu[1] + o.z * mu[2];
        }
        ray[GS2M_RAY_REC * (size_t)i + k] = o;
    }
    const float a0 = s[0] * M[2][0], a1 = s[1] * M[2][1], a2 = s[2] * M[2][2];
    const float sz = sqrtf(fmaxf(a0 * a0 + a1 * a1 + a2 * a2, 0.0f));
    const float zc = rc.y;
    ray[GS2M_RAY_REC * (size_t)i + 3] = make_float4(fmaxf(zc - 4.0f * sz, 0.2f), zc + 4.0f * sz, 0.0f, 0.0f);
}

// one component of the pixel's ray r: r.x = ray_dir(px, W, tanfovx), r.y = ray_dir(py, H, tanfovy); fp32
GS2M_DEVICE float ray_dir(const float pf, const int size, const float tanfov) {
    const float ndc = (2.0f * pf + 1.0f) / (float)size - 1.0f;
    return ndc * tanfov;
}

// z_j(p) of one staged record {w0, c0} {w1, c1} {w2, c2} {lo, hi} on the ray (rx, ry, 1); zc = the centre's view depth
GS2M_DEVICE float ray_depth(const float4 w0, const float4 w1, const float4 w2, const float4 lim, const float zc, const float rx,
                            const float ry) {
    const float u0 = fmaf(w0.x, rx, fmaf(w0.y, ry, w0.z));
    const float u1 = fmaf(w1.x, rx, fmaf(w1.y, ry, w1.z));
    const float u2 = fmaf(w2.x, rx, fmaf(w2.y, ry, w2.z));
    const float num = fmaf(w0.w, u0, fmaf(w1.w, u1, w2.w * u2));
    const float den = fmaf(u0, u0, fmaf(u1, u1, u2 * u2));
    const float q = num / den;
    const float t = (den > 0.0f && fabsf(q) <= 3.402823466e+38f) ? q : zc;
    return fminf(fmaxf(t, lim.x), lim.y);
}
