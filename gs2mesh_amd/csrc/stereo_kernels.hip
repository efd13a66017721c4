// stereo_kernels.hip -- the stereo stage (compiled with -ffp-contract=off) and its entry points:
//   k_stereo_depth_occlusion (below)  gs2m_stereo_depth_occlusion  disparity -> depth + left-right consistency mask
//   mask_kernels.h                    gs2m_mask_preprocess         the object / occlusion masks the TSDF integrates with
//   mask_disk_kernels.h               gs2m_mask_dilate_disk        disk dilation on the same bitmaps (the DTU evaluation's cull)
//   sgm_kernels.h                     gs2m_stereo_sgm              the built-in semi-global matcher
//   depth_consistency_kernels.h       gs2m_depth_consistency       the cross-view vote on the depth maps, before they are fused
//
// Depth and occlusion are the small data-parallel step between the stereo matcher and the TSDF
// (gs2mesh_utils/stereo_utils.py:132-133, 149-179).  Fused into one pass; outputs stay on the device and feed
// gs2m_tsdf_integrate directly (depth f32, mask u8) instead of going through depth.npy / occlusion_mask.npy.
//
// Per pixel (x, y), following Stereo.get_occlusion_mask's numpy arithmetic (int64 grid - float32
// disparity promotes to float64; astype(int32) truncates toward zero):
//   xp   = (int32)((double)x - L[y][x])                      x projected into the right image; a pixel whose x - L is NaN
//                                                             or outside int32 is occluded (what the reference's numpy gives
//                                                             on x86-64, where that conversion yields INT_MIN; C leaves it
//                                                             undefined and gfx950 would saturate and turn NaN into 0)
//   xc   = clip(xp, 0, W-1)
//   xr   = clip((double)xc + R[y][xc], 0, W-1)                re-projected into the left image
//   occluded = |x - xr| > threshold  or  xp < 0  or  xp >= W
//   mask = !occluded                                           (1 = visible)
//   depth = (float)(fx * baseline) / L[y][x]                   (float32 division, stereo_utils.py:133)
#include <math.h>
#include <string.h>

#include "../../include/gs2mesh_amd.h"
#include "platform.h"
#include "mask_kernels.h"
#include "mask_disk_kernels.h"
#include "sgm_kernels.h"
#include "depth_consistency_kernels.h"
#include "api_check.h"

GS2M_KERNEL void __launch_bounds__(256)
k_stereo_depth_occlusion(const float* __restrict__ disp_lr, const float* __restrict__ disp_rl, int W, int H,
                         float fb, double threshold, float* __restrict__ depth, unsigned char* __restrict__ mask) {
    const int x = (int)(blockIdx.x * 256u + threadIdx.x);
    const int y = (int)blockIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float l = disp_lr[p];
    if (depth) depth[p] = fb / l;
    if (mask) {
        const double xd = (double)x - (double)l;
        const bool in_int32 = xd > -2147483649.0 && xd < 2147483648.0;       // false for NaN
        const int xp = in_int32 ? (int)xd : -2147483647 - 1;
        const int xc = xp < 0 ? 0 : (xp > W - 1 ? W - 1 : xp);
        double xr = (double)xc + (double)disp_rl[(size_t)y * W + xc];
        xr = xr < 0.0 ? 0.0 : (xr > (double)(W - 1) ? (double)(W - 1) : xr);
        const bool occluded = fabs((double)x - xr) > threshold || xp < 0 || xp >= W;
        mask[p] = occluded ? 0 : 1;
    }
}

extern "C" int gs2m_stereo_depth_occlusion(const float* disp_lr, const float* disp_rl, int width, int height,
                                           double fx_times_baseline, double occlusion_threshold, float* depth_out,
                                           uint8_t* mask_out, gs2m_stream stream) {
    if (!disp_lr || (mask_out && !disp_rl) || width <= 0 || height <= 0) {
        gs2m_set_error("gs2m_stereo_depth_occlusion: bad argument");
        return 1;
    }
    GS2M_LAUNCH(k_stereo_depth_occlusion, dim3((width + 255) / 256, height), dim3(256), 0, stream, disp_lr, disp_rl,
                width, height, (float)fx_times_baseline, occlusion_threshold, depth_out, mask_out);
    return 0;
}

extern "C" int gs2m_mask_preprocess(int n, int width, int height, const uint8_t* const* object_masks,
                                    const uint8_t* const* occlusion_masks, int invert, int erode, int closing_k, int erosion_k,
                                    uint8_t* const* out_masks, uint64_t* scratch, gs2m_stream stream) {
    if (n < 0 || width <= 0 || height <= 0 || (n > 0 && !out_masks)) {
        gs2m_set_error("gs2m_mask_preprocess: bad argument");
        return 1;
    }
    if (closing_k < 1 || erosion_k < 1) {
        gs2m_set_error("gs2m_mask_preprocess: kernel sizes must be >= 1 (closing %d, erosion %d)", closing_k, erosion_k);
        return 1;
    }
    const size_t frame_words = (size_t)height * (size_t)((width + 63) / 64);
    for (int i = 0; i < n; ++i) {
        const bool obj = object_masks && object_masks[i], occ = occlusion_masks && occlusion_masks[i];
        if ((obj || occ) && !out_masks[i]) {
            gs2m_set_error("gs2m_mask_preprocess: frame %d has an input mask but no output", i);
            return 1;
        }
        if (obj && erode && !scratch) {
            gs2m_set_error("gs2m_mask_preprocess: the closing / erosion needs scratch");
            return 1;
        }
    }
    for (int f0 = 0; f0 < n; f0 += GS2M_MASK_BATCH) {
        const int nf = n - f0 < GS2M_MASK_BATCH ? n - f0 : GS2M_MASK_BATCH;
        MaskBatch B;
        bool any = false;
        for (int i = 0; i < GS2M_MASK_BATCH; ++i) {
            const bool in = i < nf;
            B.obj[i] = in && object_masks ? object_masks[f0 + i] : nullptr;
            B.occ[i] = in && occlusion_masks ? occlusion_masks[f0 + i] : nullptr;
            B.out[i] = in && (B.obj[i] || B.occ[i]) ? out_masks[f0 + i] : nullptr;
            any = any || B.out[i];
        }
        if (!any) continue;
        // scratch of this chunk: two bitmaps of nf frames, after those of the chunks before it
        unsigned long long* a_bits = scratch ? (unsigned long long*)scratch + 2 * (size_t)f0 * frame_words : nullptr;
        unsigned long long* b_bits = a_bits ? a_bits + (size_t)nf * frame_words : nullptr;
        gs2m_launch_mask_preprocess((hipStream_t)stream, B, nf, width, height, invert, erode, closing_k, erosion_k, a_bits, b_bits);
    }
    return 0;
}

extern "C" int gs2m_depth_consistency(int n_views, const gs2m_depth_view* views, int max_sources, const int32_t* sources,
                                      const float* pair, float rel_tol, float min_depth, float max_depth, int min_support,
                                      int max_violation, uint8_t* const* keep, uint8_t* const* support,
                                      uint8_t* const* violation, uint8_t* const* occluded, gs2m_stream stream) {
    static_assert(sizeof(ConsistencyBatch) <= 3072, "the descriptor table travels in the kernel argument segment");
    const int K = max_sources;
    if (n_views < 0 || K < 0 || K > DC_MAX_SOURCES) {
        gs2m_set_error("gs2m_depth_consistency: n_views = %d, max_sources = %d (n_views >= 0, max_sources 0 .. %d)", n_views, K,
                       DC_MAX_SOURCES);
        return 1;
    }
    if (!(rel_tol > 0.0f && rel_tol < 1.0f)) {                                             // also refuses NaN
        gs2m_set_error("gs2m_depth_consistency: rel_tol = %g must lie in (0, 1)", (double)rel_tol);
        return 1;
    }
    if (n_views == 0) return 0;
    if (!views || (K > 0 && (!sources || !pair))) {
        gs2m_set_error("gs2m_depth_consistency: NULL views, sources or pair with n_views = %d, max_sources = %d", n_views, K);
        return 1;
    }
    for (int i = 0; i < n_views; ++i) {
        const gs2m_depth_view& V = views[i];
        if (V.width <= 0 || V.height <= 0 || V.width > 65536 || V.height > 65536) {
            gs2m_set_error("gs2m_depth_consistency: view %d is %d x %d (width and height 1 .. 65536)", i, V.width, V.height);
            return 1;
        }
        if (!V.depth) {
            gs2m_set_error("gs2m_depth_consistency: view %d has a NULL depth", i);
            return 1;
        }
        for (int k = 0; k < K; ++k) {
            const int j = sources[(size_t)i * K + k];
            if (j == i || j < -1 || j >= n_views) {
                gs2m_set_error("gs2m_depth_consistency: sources[%d][%d] = %d (another view in [0, %d), or -1 for none)", i, k, j,
                               n_views);
                return 1;
            }
        }
    }
    // every argument is good: from here on the call only launches
    ConsistencyBatch B;
    int nb = 0, gw = 0, gh = 0;
    for (int i = 0; i < n_views; ++i) {
        ConsistencyRef R;
        memset(&R, 0, sizeof R);
        R.keep = keep ? keep[i] : nullptr;
        R.support = support ? support[i] : nullptr;
        R.violation = violation ? violation[i] : nullptr;
        R.occluded = occluded ? occluded[i] : nullptr;
        const bool wanted = R.keep || R.support || R.violation || R.occluded;
        if (wanted) {
            const gs2m_depth_view& V = views[i];
            R.depth = V.depth;
            R.mask = V.mask;
            R.W = V.width;
            R.H = V.height;
            R.fx = V.fx, R.fy = V.fy, R.cx = V.cx, R.cy = V.cy;
            for (int k = 0; k < K; ++k) {                                                  // the -1 entries drop out here
                const int j = sources[(size_t)i * K + k];
                if (j < 0) continue;
                ConsistencySource& S = B.src[nb][R.n_src++];
                S.depth = views[j].depth;
                S.mask = views[j].mask;
                S.W = views[j].width;
                S.H = views[j].height;
                S.fx = views[j].fx, S.fy = views[j].fy, S.cx = views[j].cx, S.cy = views[j].cy;
                memcpy(S.M, pair + ((size_t)i * K + k) * 12, sizeof S.M);
            }
            for (int k = R.n_src; k < DC_MAX_SOURCES; ++k) memset(&B.src[nb][k], 0, sizeof(ConsistencySource));
            B.ref[nb++] = R;
            gw = V.width > gw ? V.width : gw;
            gh = V.height > gh ? V.height : gh;
        }
        if (nb == DC_BATCH || (nb > 0 && i == n_views - 1)) {
            for (int b = nb; b < DC_BATCH; ++b) {                                          // unused slots: 0 x 0 views
                memset(&B.ref[b], 0, sizeof(ConsistencyRef));
                memset(B.src[b], 0, sizeof B.src[b]);
            }
            GS2M_LAUNCH(k_depth_consistency, dim3((gw + DC_PATCH_W - 1) / DC_PATCH_W, (gh + DC_PATCH_H - 1) / DC_PATCH_H, nb), dim3(256), 0,
                        stream, B, rel_tol, min_depth, max_depth, min_support, max_violation);
            nb = gw = gh = 0;
        }
    }
    return 0;
}

// the packed input masks of one chunk; the chunks of a call follow each other on the stream and share it
extern "C" int64_t gs2m_mask_dilate_disk_scratch_bytes(int n, int width, int height) {
    if (n < 0 || width <= 0 || height <= 0 || (int64_t)height * ((width + 63) / 64) > 0x7fffffffll) return -1;
    const int nf = n < GS2M_MASK_BATCH ? n : GS2M_MASK_BATCH;
    return (int64_t)nf * height * ((width + 63) / 64) * 8;
}

extern "C" int gs2m_mask_dilate_disk(int n, int width, int height, const uint8_t* const* masks, int radius, uint64_t* out_bits,
                                     uint8_t* out_bytes, void* scratch, int64_t scratch_bytes, gs2m_stream stream) {
    const int64_t need = gs2m_mask_dilate_disk_scratch_bytes(n, width, height);
    if (need < 0) {
        gs2m_set_error("gs2m_mask_dilate_disk: n = %d masks of %d x %d (n >= 0, width and height >= 1, at most 2^31 - 1 words a mask)",
                       n, width, height);
        return 1;
    }
    if (radius < 0 || radius > GS2M_DISK_MAX_RADIUS) {
        gs2m_set_error("gs2m_mask_dilate_disk: radius = %d (0 .. %d)", radius, GS2M_DISK_MAX_RADIUS);
        return 1;
    }
    if (n == 0) return 0;
    if (!masks || !out_bits) {
        gs2m_set_error("gs2m_mask_dilate_disk: NULL masks or out_bits with n = %d", n);
        return 1;
    }
    for (int i = 0; i < n; ++i)
        if (!masks[i]) {
            gs2m_set_error("gs2m_mask_dilate_disk: mask %d is NULL", i);
            return 1;
        }
    if (gs2m_scratch_refused("gs2m_mask_dilate_disk", "gs2m_mask_dilate_disk_scratch_bytes", scratch, scratch_bytes, need, 8)) return 1;
    const size_t frame_words = (size_t)height * (size_t)((width + 63) / 64);
    for (int f0 = 0; f0 < n; f0 += GS2M_MASK_BATCH) {
        const int nf = n - f0 < GS2M_MASK_BATCH ? n - f0 : GS2M_MASK_BATCH;
        gs2m_launch_mask_dilate_disk((hipStream_t)stream, masks + f0, nf, width, height, radius, (unsigned long long*)scratch,
                                     (unsigned long long*)out_bits + (size_t)f0 * frame_words,
                                     out_bytes ? out_bytes + (size_t)f0 * height * width : nullptr);
    }
    return 0;
}

extern "C" int64_t gs2m_stereo_sgm_scratch_bytes(int width, int height, int max_disparity) {
    if (width <= 0 || height <= 0 || height > 65535 || (int64_t)width * height > 0x7fffffffll || max_disparity < 64 ||
        max_disparity > 64 * SGM_MAX_K || max_disparity % 64 != 0)
        return -1;
    return sgm_scratch_layout(nullptr, width, height, max_disparity).bytes;
}

extern "C" int gs2m_stereo_sgm(const uint8_t* left_rgb8, const uint8_t* right_rgb8, int width, int height, int max_disparity,
                               int p1, int p2, float* disp_lr, float* disp_rl, void* scratch, int64_t scratch_bytes,
                               uint16_t* tap_cost_lr, gs2m_stream stream) {
    if (!left_rgb8 || !right_rgb8) {
        gs2m_set_error("gs2m_stereo_sgm: NULL image");
        return 1;
    }
    if (max_disparity < 64 || max_disparity > 64 * SGM_MAX_K || max_disparity % 64 != 0) {
        gs2m_set_error("gs2m_stereo_sgm: max_disparity must be a multiple of 64 in [64, %d], got %d", 64 * SGM_MAX_K, max_disparity);
        return 1;
    }
    const int64_t need = gs2m_stereo_sgm_scratch_bytes(width, height, max_disparity);
    if (need < 0) {
        gs2m_set_error("gs2m_stereo_sgm: unsupported image size %d x %d", width, height);
        return 1;
    }
    if (p1 <= 0 || p1 > p2 || p2 > 190) {
        gs2m_set_error("gs2m_stereo_sgm: penalties must satisfy 0 < p1 <= p2 <= 190, got p1 = %d, p2 = %d", p1, p2);
        return 1;
    }
    if (gs2m_scratch_refused("gs2m_stereo_sgm", "gs2m_stereo_sgm_scratch_bytes", scratch, scratch_bytes, need, 1)) return 1;
    if (((uintptr_t)scratch | (uintptr_t)tap_cost_lr) & 15u) {                // one message for both pointers
        gs2m_set_error("gs2m_stereo_sgm: scratch and tap_cost_lr must be 16-byte aligned");
        return 1;
    }
    if (!disp_lr && !disp_rl && !tap_cost_lr) return 0;
    sgm_launch((hipStream_t)stream, left_rgb8, right_rgb8, width, height, max_disparity, p1, p2, disp_lr, disp_rl,
               sgm_scratch_layout(scratch, width, height, max_disparity), tap_cost_lr);
    return 0;
}

// A build list from before the split names only this file and gets the point-set and training entry points through it;
// one that compiles the two units itself says so with -DGS2M_SPLIT_UNITS (build.py, tests/emu/build_emu.py).
#ifndef GS2M_SPLIT_UNITS
#include "points_kernels.hip"
#include "train_kernels.hip"
#endif
