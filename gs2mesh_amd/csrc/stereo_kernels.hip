// stereo_kernels.hip -- disparity -> depth + left-right consistency mask, the small
// data-parallel step between the stereo network and the TSDF (gs2mesh_utils/stereo_utils.py:132-133,
// 149-179).  Fused into one pass; outputs stay on the device and feed gs2m_tsdf_integrate directly
// (depth f32, mask u8) instead of going through depth.npy / occlusion_mask.npy.
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
#include "sgm_kernels.h"
#include "knn_kernels.h"
#include "nn_kernels.h"
#include "mesh_sample_kernels.h"
#include "device_memory.h"
#include "loss_kernels.h"
#include "optim_kernels.h"

void gs2m_set_error(const char* fmt, ...);
void gs2m_launch_scan_u32(hipStream_t st, const unsigned* in, unsigned n, unsigned* out, unsigned* scratch);    // tsdf_kernels.hip

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
    if (!scratch || scratch_bytes < need) {
        gs2m_set_error("gs2m_stereo_sgm: scratch of %lld bytes, gs2m_stereo_sgm_scratch_bytes asks for %lld",
                       (long long)(scratch ? scratch_bytes : 0), (long long)need);
        return 1;
    }
    if (((uintptr_t)scratch | (uintptr_t)tap_cost_lr) & 15u) {
        gs2m_set_error("gs2m_stereo_sgm: scratch and tap_cost_lr must be 16-byte aligned");
        return 1;
    }
    if (!disp_lr && !disp_rl && !tap_cost_lr) return 0;
    sgm_launch((hipStream_t)stream, left_rgb8, right_rgb8, width, height, max_disparity, p1, p2, disp_lr, disp_rl,
               sgm_scratch_layout(scratch, width, height, max_disparity), tap_cost_lr);
    return 0;
}

extern "C" int64_t gs2m_knn_scratch_bytes(int P) { return P <= 0 ? 0 : knn_scratch_layout(nullptr, P).bytes; }

extern "C" int gs2m_knn_mean_dist2(int P, const float* points, const int32_t* order, void* scratch, int64_t scratch_bytes,
                                   float* out, gs2m_stream stream) {
    if (P < 0) {
        gs2m_set_error("gs2m_knn_mean_dist2: P = %d", P);
        return 1;
    }
    if (P == 0) return 0;
    if (!points || !out) {
        gs2m_set_error("gs2m_knn_mean_dist2: NULL points or out with P = %d", P);
        return 1;
    }
    const int64_t need = gs2m_knn_scratch_bytes(P);
    if (!scratch || scratch_bytes < need) {
        gs2m_set_error("gs2m_knn_mean_dist2: scratch of %lld bytes, gs2m_knn_scratch_bytes asks for %lld",
                       (long long)(scratch ? scratch_bytes : 0), (long long)need);
        return 1;
    }
    if ((uintptr_t)scratch & 15u) {
        gs2m_set_error("gs2m_knn_mean_dist2: scratch must be 16-byte aligned");
        return 1;
    }
    knn_launch((hipStream_t)stream, P, points, order, knn_scratch_layout(scratch, P), out);
    return 0;
}

extern "C" int64_t gs2m_nn_scratch_bytes(int Q, int R) {
    (void)Q;                                                          // only the references are copied and boxed
    return R <= 0 ? 0 : knn_scratch_layout(nullptr, R).bytes;
}

extern "C" int gs2m_nn_dist2(int Q, const float* queries, const int32_t* query_order, int R, const float* refs,
                             const int32_t* ref_order, void* scratch, int64_t scratch_bytes, float* out_d2, int32_t* out_idx,
                             gs2m_stream stream) {
    if (Q < 0 || R < 0) {
        gs2m_set_error("gs2m_nn_dist2: Q = %d, R = %d", Q, R);
        return 1;
    }
    if (Q == 0) return 0;
    if (!queries || !out_d2) {
        gs2m_set_error("gs2m_nn_dist2: NULL queries or out_d2 with Q = %d", Q);
        return 1;
    }
    if (R > 0) {
        if (!refs) {
            gs2m_set_error("gs2m_nn_dist2: NULL refs with R = %d", R);
            return 1;
        }
        const int64_t need = gs2m_nn_scratch_bytes(Q, R);
        if (!scratch || scratch_bytes < need) {
            gs2m_set_error("gs2m_nn_dist2: scratch of %lld bytes, gs2m_nn_scratch_bytes asks for %lld",
                           (long long)(scratch ? scratch_bytes : 0), (long long)need);
            return 1;
        }
        if ((uintptr_t)scratch & 15u) {
            gs2m_set_error("gs2m_nn_dist2: scratch must be 16-byte aligned");
            return 1;
        }
    }
    nn_launch((hipStream_t)stream, Q, queries, query_order, R, refs, ref_order, knn_scratch_layout(R > 0 ? scratch : nullptr, R), out_d2,
              out_idx);
    return 0;
}

// 0: nothing to do, 1: refused (the message is set), 2: go
static int mesh_sample_check(const char* fn, int64_t n_vertices, const double* vertices, int64_t n_triangles, const int32_t* triangles) {
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > 0x7fffffffll || n_triangles > 0x7fffffffll) {
        gs2m_set_error("%s: %lld vertices, %lld triangles (each 0 .. 2^31 - 1)", fn, (long long)n_vertices, (long long)n_triangles);
        return 1;
    }
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) {
        gs2m_set_error("%s: NULL vertices or triangles", fn);
        return 1;
    }
    return n_triangles == 0 ? 0 : 2;
}

extern "C" int gs2m_mesh_sample_count(int64_t n_vertices, const double* vertices, int64_t n_triangles, const int32_t* triangles,
                                      double density, uint32_t* counts, uint32_t* offsets, void* state, int64_t state_bytes,
                                      gs2m_stream stream, int64_t* total, uint32_t* status) {
    if (!total || !status) {
        gs2m_set_error("gs2m_mesh_sample_count: NULL total or status");
        return 1;
    }
    *total = 0;
    *status = 0;
    const int go = mesh_sample_check("gs2m_mesh_sample_count", n_vertices, vertices, n_triangles, triangles);
    if (go != 2) return go;
    if (!counts || !offsets) {
        gs2m_set_error("gs2m_mesh_sample_count: NULL counts or offsets with %lld triangles", (long long)n_triangles);
        return 1;
    }
    const int64_t need = GS2M_MESH_SAMPLE_STATE_BYTES(n_triangles);
    if (!state || state_bytes < need || ((uintptr_t)state & 7u)) {
        gs2m_set_error("gs2m_mesh_sample_count: state of %lld bytes, GS2M_MESH_SAMPLE_STATE_BYTES asks for %lld, 8-byte aligned",
                       (long long)(state ? state_bytes : 0), (long long)need);
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)n_triangles;
    unsigned long long* words = (unsigned long long*)state;
    GS2M_HIPCHK(hipMemsetAsync(words, 0, 16, st));
    GS2M_LAUNCH(k_mesh_sample_count, dim3((nt + 255u) / 256u), dim3(256), 0, st, (unsigned)n_vertices, vertices, triangles, nt, density,
                counts, words);
    gs2m_launch_scan_u32(st, counts, nt, offsets, (unsigned*)(words + 2));
    unsigned long long h[2] = {0ull, 0ull};
    GS2M_HIPCHK(hipMemcpyAsync(h, words, 16, hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    GS2M_HIPCHK(hipGetLastError());
    *status = (uint32_t)h[1] | (h[0] > 0x7fffffffull ? GS2M_MESH_SAMPLE_TOTAL : 0u);
    *total = (int64_t)h[0];
    return 0;
}

extern "C" int gs2m_mesh_sample_emit(int64_t n_vertices, const double* vertices, int64_t n_triangles, const int32_t* triangles,
                                     double density, const uint32_t* counts, const uint32_t* offsets, int64_t total, double* points,
                                     gs2m_stream stream) {
    const int go = mesh_sample_check("gs2m_mesh_sample_emit", n_vertices, vertices, n_triangles, triangles);
    if (go == 1) return 1;
    if (total < 0 || total > 0x7fffffffll || (go == 0 && total != 0)) {
        gs2m_set_error("gs2m_mesh_sample_emit: total = %lld with %lld triangles", (long long)total, (long long)n_triangles);
        return 1;
    }
    if (n_vertices + total == 0) return 0;
    if (!points || (go == 2 && (!counts || !offsets))) {
        gs2m_set_error("gs2m_mesh_sample_emit: NULL points, counts or offsets");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_vertices > 0)
        GS2M_HIPCHK(hipMemcpyAsync(points, vertices, sizeof(double) * 3 * (size_t)n_vertices, hipMemcpyDeviceToDevice, st));
    if (go == 2 && total > 0) {
        const unsigned nt = (unsigned)n_triangles;
        GS2M_LAUNCH(k_mesh_sample_emit, dim3((nt + 255u) / 256u), dim3(256), 0, st, (unsigned)n_vertices, vertices, triangles, nt, density,
                    counts, offsets, (unsigned long long)total, points);
    }
    return 0;
}

// 0: nothing to do, 1: refused (the message is set), 2: go
static int loss_check_sizes(const char* fn, int planes, int height, int width) {
    if (planes < 0 || height < 0 || width < 0) {
        gs2m_set_error("%s: negative %s (%d x %d x %d)", fn, planes < 0 ? "planes" : height < 0 ? "height" : "width", planes, height,
                       width);
        return 1;
    }
    if (planes == 0 || height == 0 || width == 0) return 0;
    if (const int64_t tiles = loss_tiling(planes, height, width).tiles; tiles <= 0 || tiles > LOSS_MAX_TILES) {
        gs2m_set_error("%s: size %d x %d x %d is more than %d tiles of %d x %d", fn, planes, height, width, LOSS_MAX_TILES,
                       LOSS_TW, LOSS_TH);
        return 1;
    }
    return 2;
}

extern "C" int64_t gs2m_photo_loss_scratch_bytes(int planes, int height, int width) {
    if (planes <= 0 || height <= 0 || width <= 0) return 0;
    const int64_t tiles = loss_tiling(planes, height, width).tiles;
    return tiles <= 0 || tiles > LOSS_MAX_TILES ? -1 : 16 * ((tiles + 1) / 2);                        // a pair of floats per tile
}

extern "C" int gs2m_photo_loss_forward(int planes, int height, int width, const float* image, const float* target,
                                       float lambda_dssim, void* scratch, int64_t scratch_bytes, float* out, float* partials,
                                       float* tap_map, gs2m_stream stream) {
    const int go = loss_check_sizes("gs2m_photo_loss_forward", planes, height, width);
    if (go != 2) return go;
    if (!image || !target || !out) {
        gs2m_set_error("gs2m_photo_loss_forward: NULL %s", !image ? "image" : !target ? "target" : "out");
        return 1;
    }
    const int64_t need = gs2m_photo_loss_scratch_bytes(planes, height, width);
    if (!scratch || scratch_bytes < need) {
        gs2m_set_error("gs2m_photo_loss_forward: scratch of %lld bytes, gs2m_photo_loss_scratch_bytes asks for %lld",
                       (long long)(scratch ? scratch_bytes : 0), (long long)need);
        return 1;
    }
    if ((uintptr_t)scratch & 15u) {
        gs2m_set_error("gs2m_photo_loss_forward: scratch must be 16-byte aligned");
        return 1;
    }
    loss_launch_forward((hipStream_t)stream, planes, height, width, image, target, lambda_dssim, (float*)scratch, out, partials,
                        tap_map);
    return 0;
}

extern "C" int gs2m_photo_loss_backward(int planes, int height, int width, const float* image, const float* target,
                                        const float* partials, float lambda_dssim, const float* grad_loss, float* grad_image,
                                        gs2m_stream stream) {
    const int go = loss_check_sizes("gs2m_photo_loss_backward", planes, height, width);
    if (go != 2) return go;
    if (!image || !target || !partials || !grad_loss || !grad_image) {
        gs2m_set_error("gs2m_photo_loss_backward: NULL %s", !image ? "image" : !target ? "target" : !partials ? "partials"
                                                                 : !grad_loss ? "grad_loss" : "grad_image");
        return 1;
    }
    loss_launch_backward((hipStream_t)stream, planes, height, width, image, target, partials, lambda_dssim, grad_loss, grad_image);
    return 0;
}

extern "C" int gs2m_adam_step(int n_segments, const gs2m_adam_segment* segments, const int32_t* row_visible, int64_t rows,
                              gs2m_stream stream) {
    const char* fn = "gs2m_adam_step";
    if (n_segments < 1 || n_segments > ADAM_MAX_SEGMENTS) {
        gs2m_set_error("%s: n_segments must be in [1, %d], got %d", fn, ADAM_MAX_SEGMENTS, n_segments);
        return 1;
    }
    if (!segments) {
        gs2m_set_error("%s: NULL segments", fn);
        return 1;
    }
    if (row_visible && rows < 0) {
        gs2m_set_error("%s: rows = %lld", fn, (long long)rows);
        return 1;
    }
    AdamTable T;
    memset(&T, 0, sizeof(T));
    struct Range {
        uintptr_t lo, hi;
        int segment;
        const char* name;
    } ranges[4 * ADAM_MAX_SEGMENTS + 1];
    int n_ranges = 0;
    uint64_t wgs = 0;
    for (int i = 0; i < n_segments; ++i) {
        const gs2m_adam_segment& a = segments[i];
        if (a.count < 0) {
            gs2m_set_error("%s: segment %d: count = %lld", fn, i, (long long)a.count);
            return 1;
        }
        if (a.row_width < 1) {
            gs2m_set_error("%s: segment %d: row_width must be >= 1, got %d", fn, i, a.row_width);
            return 1;
        }
        if (a.step < 1) {
            gs2m_set_error("%s: segment %d: step must be >= 1 (the step being taken), got %lld", fn, i, (long long)a.step);
            return 1;
        }
        if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0)) {
            gs2m_set_error("%s: segment %d: betas must be in [0, 1), got %g and %g", fn, i, a.beta1, a.beta2);
            return 1;
        }
        if (row_visible && (a.count / a.row_width != rows || a.count % a.row_width != 0)) {
            gs2m_set_error("%s: segment %d: count %lld is not rows x row_width = %lld x %d", fn, i, (long long)a.count,
                           (long long)rows, a.row_width);
            return 1;
        }
        if (a.count == 0) continue;
        if (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq) {
            gs2m_set_error("%s: segment %d: NULL %s with count = %lld", fn, i,
                           !a.param ? "param" : !a.grad ? "grad" : !a.exp_avg ? "exp_avg" : "exp_avg_sq", (long long)a.count);
            return 1;
        }
        if (a.count > (int64_t)0x7fffffff * ADAM_WG_ELEMS) {
            gs2m_set_error("%s: segment %d: count %lld is more than 2^31 - 1 workgroups of %d elements", fn, i, (long long)a.count,
                           ADAM_WG_ELEMS);
            return 1;
        }
        const void* ptrs[4] = {a.param, a.grad, a.exp_avg, a.exp_avg_sq};
        const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int k = 0; k < 4; ++k)
            ranges[n_ranges++] = Range{(uintptr_t)ptrs[k], (uintptr_t)ptrs[k] + 4 * (uintptr_t)a.count, i, names[k]};
        AdamSegment& s = T.seg[T.n];
        s.p = a.param, s.g = a.grad, s.m = a.exp_avg, s.v = a.exp_avg_sq;
        s.count = a.count;
        s.row_width = a.row_width;
        s.vec = (((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15u) == 0;
        adam_scalars(s, a.lr, a.beta1, a.beta2, a.eps, a.step);
        T.first_wg[T.n++] = (unsigned)wgs;
        wgs += (uint64_t)((a.count + ADAM_WG_ELEMS - 1) / ADAM_WG_ELEMS);
        if (wgs > 0x7fffffffull) {
            gs2m_set_error("%s: the call needs more than 2^31 - 1 workgroups of %d elements", fn, ADAM_WG_ELEMS);
            return 1;
        }
    }
    if (T.n == 0) return 0;
    if (row_visible) ranges[n_ranges++] = Range{(uintptr_t)row_visible, (uintptr_t)row_visible + 4 * (uintptr_t)rows, -1, "row_visible"};
    for (int i = 0; i < n_ranges; ++i)
        for (int j = i + 1; j < n_ranges; ++j)
            if (ranges[i].lo < ranges[j].hi && ranges[j].lo < ranges[i].hi) {
                gs2m_set_error("%s: %s of segment %d overlaps %s of segment %d", fn, ranges[i].name, ranges[i].segment,
                               ranges[j].name, ranges[j].segment);
                return 1;
            }
    for (int k = T.n; k <= ADAM_MAX_SEGMENTS; ++k) T.first_wg[k] = ADAM_NO_WG;
    GS2M_LAUNCH(k_adam_multi, dim3((unsigned)wgs), dim3(ADAM_THREADS), 0, stream, T, (const int*)row_visible);
    return 0;
}

extern "C" int gs2m_densify_stats(int P, const int32_t* radii, const float* viewspace_grad, float* max_radii2D, float* grad_accum,
                                  float* denom, gs2m_stream stream) {
    if (P < 0) {
        gs2m_set_error("gs2m_densify_stats: P = %d", P);
        return 1;
    }
    if (P == 0) return 0;
    if (!radii || !viewspace_grad || !max_radii2D || !grad_accum || !denom) {
        gs2m_set_error("gs2m_densify_stats: NULL %s with P = %d", !radii ? "radii" : !viewspace_grad ? "viewspace_grad"
                                                                  : !max_radii2D ? "max_radii2D" : !grad_accum ? "grad_accum"
                                                                                                 : "denom", P);
        return 1;
    }
    GS2M_LAUNCH(k_densify_stats, dim3((unsigned)(((int64_t)P + 255) / 256)), dim3(256), 0, stream, P, (const int*)radii,
                viewspace_grad, max_radii2D, grad_accum, denom);
    return 0;
}
