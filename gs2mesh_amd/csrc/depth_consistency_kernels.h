// depth_consistency_kernels.h -- gs2m_depth_consistency: the cross-view test between the depth stage and the TSDF.  Every valid
// pixel of a reference view is lifted with its depth, carried into up to 16 source views and compared with the depth the
// source holds there: the source supports the pixel, sees past it (violation: the point lies in the source's observed free
// space) or sees something in front of it (occluded: no evidence).  include/gs2mesh_amd.h states the arithmetic, operation by
// operation in f32 (this header is compiled into stereo_kernels.hip, built with -ffp-contract=off);
// tests/consistency_statement.py restates it in numpy.
//
// k_depth_consistency:
//   Table.   The descriptors of a launch are the kernel argument, by value (ConsistencyBatch, 2976 bytes of the kernarg
//            segment, as k_adam_multi's segment table): there is no device-side table and no host-to-device copy, so the call
//            is asynchronous on its stream and needs no scratch.  A launch carries DC_BATCH reference views along
//            blockIdx.z, each with its own (compacted: no -1) source list; the grid covers the largest view of the launch
//            and the workgroups past a smaller view's edge leave at once.
//   Layout.  One lane per reference pixel, the sources in a loop, the three counts in registers.  A wave is a 16 x 4 patch of
//            pixels, not a 64-pixel row segment, and a 256-lane workgroup 2 x 2 of them: 32 x 8 pixels.  The neighbour's camera
//            is rotated against this one, so a row segment's gather into the source map can spread over up to 64 lines when
//            the rotation has a roll component, while a patch's stays within a few rows of about 64 bytes either way; the
//            workgroup's rows are 128 bytes of the reference depth, one cache line.  On a ring without roll (the best case
//            for row segments) the patch and the row segment measured alike, and 16-pixel-wide workgroups 6 % or more
//            behind the 32-wide one; a scene with roll was not measured (DESIGN.md 4d has the table and what it supports).
//   Access.  The reference depth is read once, 64 bytes of four rows per wave; the four outputs are plain byte stores in
//            16-byte runs per wave, 32-byte runs per workgroup.  Descriptors are indexed by blockIdx.z and the loop counter
//            alone, so they are scalar loads.  No LDS, no atomics: one lane owns each pixel, the same bits every run.
//   Bounds.  A source pixel is read only after `pu >= 0 && pu < (float)W && pv >= 0 && pv < (float)H` (false for NaN); W and
//            H are at most 65536 (the entry point refuses more), so the converts are exact, floorf(pu) <= W - 1 and the grid
//            stays inside HIP's limits.
#pragma once
#include <math.h>

#include "platform.h"

#define DC_MAX_SOURCES 16
#define DC_BATCH 2                        // reference views per launch (blockIdx.z)
#define DC_WAVE_W 16                      // a wave is 16 x 4 pixels,
#define DC_WAVE_H 4
#define DC_PATCH_W (2 * DC_WAVE_W)        // a workgroup 2 x 2 waves: 32 x 8
#define DC_PATCH_H (2 * DC_WAVE_H)

struct ConsistencySource {                // 88 bytes
    const float* depth;
    const unsigned char* mask;
    int W, H;
    float fx, fy, cx, cy;
    float M[12];                          // reference camera -> this camera, row-major 3 x 4
};

struct ConsistencyRef {                   // 80 bytes
    const float* depth;
    const unsigned char* mask;
    unsigned char* keep;
    unsigned char* support;
    unsigned char* violation;
    unsigned char* occluded;
    int W, H;                             // 0 x 0: an unused slot of the launch
    float fx, fy, cx, cy;
    int n_src;
    int reserved;
};

struct ConsistencyBatch {
    ConsistencyRef ref[DC_BATCH];
    ConsistencySource src[DC_BATCH][DC_MAX_SOURCES];
};

GS2M_DEVICE bool dc_depth_valid(float d, float min_depth, float max_depth) {
    return d > 0.0f && d >= min_depth && d < max_depth;                                    // false for NaN
}

GS2M_KERNEL void __launch_bounds__(256)
k_depth_consistency(ConsistencyBatch T, float rel_tol, float min_depth, float max_depth, int min_support, int max_violation) {
    const int z = (int)blockIdx.z;
    const ConsistencyRef& R = T.ref[z];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int u = (int)blockIdx.x * DC_PATCH_W + (wave & 1) * DC_WAVE_W + lane % DC_WAVE_W;
    const int v = (int)blockIdx.y * DC_PATCH_H + (wave >> 1) * DC_WAVE_H + lane / DC_WAVE_W;
    if (u >= R.W || v >= R.H) return;
    const size_t p = (size_t)v * (size_t)R.W + (size_t)u;
    const float d = R.depth[p];
    const bool valid = dc_depth_valid(d, min_depth, max_depth) && (!R.mask || R.mask[p] != 0);
    int support = 0, violation = 0, occluded = 0;
    if (valid) {
        const float x = (((float)u - R.cx) * d) / R.fx;
        const float y = (((float)v - R.cy) * d) / R.fy;
        const int n_src = R.n_src;
        for (int k = 0; k < n_src; ++k) {
            const ConsistencySource& S = T.src[z][k];
            const float* m = S.M;
            const float q0 = ((m[0] * x + m[1] * y) + m[2] * d) + m[3];
            const float q1 = ((m[4] * x + m[5] * y) + m[6] * d) + m[7];
            const float q2 = ((m[8] * x + m[9] * y) + m[10] * d) + m[11];
            if (!(q2 > 0.0f)) continue;
            const float pu = ((q0 * S.fx) / q2 + S.cx) + 0.5f;
            const float pv = ((q1 * S.fy) / q2 + S.cy) + 0.5f;
            if (!(pu >= 0.0f && pu < (float)S.W && pv >= 0.0f && pv < (float)S.H)) continue;      // false for NaN
            const int iu = (int)floorf(pu), iv = (int)floorf(pv);
            const size_t sp = (size_t)iv * (size_t)S.W + (size_t)iu;
            const float ds = S.depth[sp];
            if (!dc_depth_valid(ds, min_depth, max_depth)) continue;
            if (S.mask && S.mask[sp] == 0) continue;
            const float diff = ds - q2, tol = rel_tol * q2;
            if (fabsf(diff) <= tol)
                ++support;
            else if (diff > tol)
                ++violation;
            else
                ++occluded;
        }
    }
    if (R.keep) R.keep[p] = valid && support >= min_support && violation <= max_violation ? 1 : 0;
    if (R.support) R.support[p] = (unsigned char)support;
    if (R.violation) R.violation[p] = (unsigned char)violation;
    if (R.occluded) R.occluded[p] = (unsigned char)occluded;
}
