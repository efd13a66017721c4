// train_kernels.hip -- the training kernels (compiled with -ffp-contract=off: their headers promise every operation
// rounded on its own) and their entry points:
//   loss_kernels.h   gs2m_photo_loss_*                     fused L1 + D-SSIM loss, forward and backward
//   optim_kernels.h  gs2m_adam_step, gs2m_densify_stats    the Adam step over up to 8 tensors; densification statistics
#include <math.h>
#include <string.h>

#include "../../include/gs2mesh_amd.h"
#include "platform.h"
#include "loss_kernels.h"
#include "optim_kernels.h"
#include "api_check.h"

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
    if (gs2m_scratch_refused("gs2m_photo_loss_forward", "gs2m_photo_loss_scratch_bytes", scratch, scratch_bytes,
                             gs2m_photo_loss_scratch_bytes(planes, height, width), 16))
        return 1;
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
