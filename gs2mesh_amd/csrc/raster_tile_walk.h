// raster_tile_walk.h -- the front-to-back walk of one 16 x 16 tile's sorted list by one wave, stated once for k_blend_depth
// (raster_depth.h) and walk 1 of k_blend_backward (raster_backward_blend.h): the prologue (walk_tile), the batch gather
// (walk_gather) and the step at one pixel (walk_step).  Both kernels run THIS step in one translation unit (raster_blend.hip), and
// the step leaves no contraction choice to the compiler -- alpha by bw_alpha's explicit FMAs, then
//     w = alpha * T (a product rounded on its own);   S = fmaf(T, alpha, S) (NOT S + w);   Z = fmaf(w, z, Z)
// -- so the backward's D = Z / S has the depth pass's bits and its median is the depth pass's instance.
#pragma once
#include "raster_common.h"

// alpha of one staged instance at one pixel: renderCUDA's `power`, G = exp(power), alpha = min(0.99, o G) and the two skip
// decisions (forward.cu:331-343 = backward.cu:491-501).  Explicit FMAs: every walk of every kernel rounds alike.
GS2M_DEVICE bool bw_alpha(const float4 A, const float4 B, const float pxf, const float pyf, float& dx, float& dy, float& G,
                          float& alpha) {
    dx = A.x - pxf;
    dy = A.y - pyf;
    const float power = fmaf(-0.5f * A.z * dx, dx, fmaf(-0.5f * B.x * dy, dy, -(A.w * dx) * dy));
    G = gs2m_fast_exp(power);
    alpha = fminf(0.99f, B.y * G);
    return !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
}

// what a wave knows of its tile before it walks the list; pixel k of the lane is quadrant (k & 1, k >> 1) of the tile
struct TileWalk {
    int wave, lane, tx, ty;
    unsigned r0, r1;           // the tile's list is keys[r0, r1): clamped to the instance arena, wave-uniform
    int x[4], y[4];
    float pxf[4], pyf[4];
    bool inside[4];            // pixel k lies inside the W x H image
};

// grid: ceil(tiles / WPB) workgroups of WPB waves; wave w of workgroup b walks tile b * WPB + w (a wave past the last tile has
// none: the kernel returns before walk_tile reads the tile's range)
template <int WPB>
GS2M_DEVICE int walk_tile_of_wave() { return gs2m_uniform((int)blockIdx.x * WPB + (int)(threadIdx.x >> 6)); }

GS2M_DEVICE TileWalk walk_tile(const int tile, const unsigned* __restrict__ tile_start, const unsigned cap, const int W,
                               const int H, const int gx) {
    TileWalk t;
    t.wave = (int)(threadIdx.x >> 6);
    t.lane = (int)(threadIdx.x & 63u);
    t.ty = tile / gx;
    t.tx = tile - t.ty * gx;
    unsigned r0, r1;
    gs2m_list_range(tile_start, tile, cap, r0, r1);   // tile_start is this view's own row
    t.r0 = (unsigned)gs2m_uniform((int)r0);
    t.r1 = (unsigned)gs2m_uniform((int)r1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.x[k] = t.tx * GS2M_TILE + (t.lane & 7) + 8 * (k & 1);
        t.y[k] = t.ty * GS2M_TILE + (t.lane >> 3) + 8 * (k >> 1);
        t.inside[k] = t.x[k] < W && t.y[k] < H;
        t.pxf[k] = (float)t.x[k];
        t.pyf[k] = (float)t.y[k];
    }
    return t;
}

// The 64 instances [base, base + 64) of the list -> LDS (lane l stages instance base + l): a = {mx, my, ca, cb},
// b = {cc, op, r, g} and, with WANT_Z, the view-space depth of the centre.  extra(gid, rc) runs for the staging lane with the
// guarded id and its third record {b, z, rect0, rect1}: what else a kernel stages.  An id the forward cannot have written
// stages record 0 with opacity 0 and z 0, in every kernel (opacity 0 skips the instance before any walk reads its z).
template <bool WANT_Z, class Extra>
GS2M_DEVICE void walk_gather(const TileWalk& t, const unsigned base, const unsigned long long* __restrict__ keys,
                             const GeomRecs recs, const int P, float4* sa, float4* sb, float* sz, const Extra extra) {
    gs2m_wave_sync();   // the previous batch has been read by every lane
    if (base + (unsigned)t.lane < t.r1) {
        unsigned gid = (unsigned)(keys[base + t.lane] & 0xffffffffull);
        const bool known = gid < (unsigned)P;   // never index the records with an id the forward cannot have written
        gid = known ? gid : 0u;
        const float4 ra = recs.ab[2 * (size_t)gid], rc = recs.c[gid];
        float4 rb = recs.ab[2 * (size_t)gid + 1];
        if (!known) rb.y = 0.0f;   // opacity 0: alpha < 1/255 everywhere, the instance is skipped by every walk
        sa[t.lane] = ra;
        sb[t.lane] = rb;
        extra(gid, rc);
        if constexpr (WANT_Z) sz[t.lane] = known ? rc.y : 0.0f;
    }
    gs2m_wave_sync();
}

// One staged instance (A, B, depth z) at one pixel, front to back.  When the pixel accepts the instance, T becomes the
// transmittance behind it.  CARRY: S and Z accumulate, and `med` (0 = not yet) takes `med_rec` when the instance is the first to
// take T to one half or below; without CARRY none of S, Z, med and med_rec is read or written.  COUNT: *n_contrib takes `pos`,
// the list position after the instance; without COUNT neither is read.
template <bool CARRY, bool COUNT, class M>
GS2M_DEVICE void walk_step(const float4 A, const float4 B, const float z, const float pxf, const float pyf, float& T, bool& done,
                           float& S, float& Z, M& med, const M med_rec, int* n_contrib, const int pos) {
    float dx, dy, G, alpha;
    const bool ok = bw_alpha(A, B, pxf, pyf, dx, dy, G, alpha) && !done;
    const float test_T = T * (1.0f - alpha);
    const bool sat = ok && test_T < 0.0001f;     // stop BEFORE accumulating (forward.cu:345-350)
    done = done || sat;
    if (ok && !sat) {
        if constexpr (CARRY) {
            const float w = alpha * T;
            S = fmaf(T, alpha, S);
            Z = fmaf(w, z, Z);
            if (med == M(0) && test_T <= 0.5f) med = med_rec;
        }
        T = test_T;
        if constexpr (COUNT) *n_contrib = pos;
    }
}
