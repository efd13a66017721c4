// points_cull_kernels.h -- the per-view vertex cull of the DTU evaluation's cull_scan
// (evaluation/DTU/eval_code/evaluate_single_scene.py:63-99): every point is projected into every view and kept iff, in each
// view, it lands outside the image or on that view's (dilated) mask.  The arithmetic is the reference's, operation by
// operation in f32 (this unit is compiled with -ffp-contract=off), and the sampling is torch's grid_sampler for
// mode='nearest', padding_mode='zeros', align_corners=True; include/gs2mesh_amd.h states both.
//
// One thread per point, a loop over the views that ends at the first view that fails.  The projection rows are read with a
// wave-uniform index (scalar loads); the bitmaps of a whole scan (64 views of 1600 x 1200: 12 MB) stay in the caches.
#pragma once
#include <math.h>

#include "platform.h"

GS2M_KERNEL void __launch_bounds__(256)
k_points_cull_views(int V, const float* __restrict__ points, int n_views, const float* __restrict__ proj,
                    const unsigned long long* __restrict__ bits, int Wm, int Hm, int nw, float norm_w, float norm_h,
                    unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    const float nw1 = norm_w - 1.0f, nh1 = norm_h - 1.0f;
    const float sw = (float)(Wm - 1), sh = (float)(Hm - 1);
    bool ok = true;
    for (int v = 0; v < n_views && ok; ++v) {
        const float* m = proj + 12 * (size_t)v;
        const float c0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        const float c1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        const float c2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        const float den = c2 + 1e-6f;
        const float pu = c0 / den, pv = c1 / den;
        const float gx = (pu / nw1 - 0.5f) * 2.0f, gy = (pv / nh1 - 0.5f) * 2.0f;
        const bool valid = gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;            // false when anything is NaN
        const float fx = rintf(((gx + 1.0f) / 2.0f) * sw), fy = rintf(((gy + 1.0f) / 2.0f) * sh);   // ties to even
        bool s = false;
        if (fx >= 0.0f && fx < (float)Wm && fy >= 0.0f && fy < (float)Hm) {              // false for NaN and +-inf
            const int ix = (int)fx, iy = (int)fy;
            s = (bits[((size_t)v * Hm + iy) * nw + (ix >> 6)] >> (ix & 63)) & 1ull;
        }
        ok = s || !valid;
    }
    keep[i] = ok ? 1 : 0;
}
