// points_kernels.hip -- the point-set kernels (compiled with -ffp-contract=off: their headers promise every operation
// rounded on its own) and their entry points:
//   knn_kernels.h          gs2m_knn_*          mean squared distance to the three nearest neighbours (simple_knn's distCUDA2)
//   nn_kernels.h           gs2m_nn_*           nearest reference of every query (mesh evaluation); shares knn_scratch_layout
//   mesh_sample_kernels.h  gs2m_mesh_sample_*  points on the surface of a triangle mesh (mesh evaluation)
//   points_cull_kernels.h  gs2m_points_cull_views  keep-mask of a point set against the masks of all views (DTU's cull_scan)
//   icp_kernels.h          gs2m_icp_*, gs2m_voxel_mean  one ICP iteration on f64 point sets over nn_kernels.h's walk; voxel means
#include <math.h>
#include <string.h>

#include "../../include/gs2mesh_amd.h"
#include "platform.h"
#include "knn_kernels.h"
#include "nn_kernels.h"
#include "mesh_sample_kernels.h"
#include "points_cull_kernels.h"
#include "icp_kernels.h"
#include "api_check.h"
#include "tsdf_internal.h"          // gs2m_launch_scan_u32

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
    if (gs2m_scratch_refused("gs2m_knn_mean_dist2", "gs2m_knn_scratch_bytes", scratch, scratch_bytes, gs2m_knn_scratch_bytes(P), 16))
        return 1;
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
        if (gs2m_scratch_refused("gs2m_nn_dist2", "gs2m_nn_scratch_bytes", scratch, scratch_bytes, gs2m_nn_scratch_bytes(Q, R), 16))
            return 1;
    }
    nn_launch((hipStream_t)stream, Q, queries, query_order, R, refs, ref_order, knn_scratch_layout(R > 0 ? scratch : nullptr, R), out_d2,
              out_idx);
    return 0;
}

extern "C" int64_t gs2m_icp_scratch_bytes(int N, int R) { return icp_scratch_layout(nullptr, N, R).bytes; }

extern "C" int gs2m_icp_prepare(int R, const double* target, const double* origin, const int32_t* ref_order, void* scratch,
                                int64_t scratch_bytes, gs2m_stream stream) {
    if (R < 0) {
        gs2m_set_error("gs2m_icp_prepare: R = %d", R);
        return 1;
    }
    if (R == 0) return 0;
    if (!target || !origin) {
        gs2m_set_error("gs2m_icp_prepare: NULL target or origin with R = %d", R);
        return 1;
    }
    if (gs2m_scratch_refused("gs2m_icp_prepare", "gs2m_icp_scratch_bytes", scratch, scratch_bytes, gs2m_icp_scratch_bytes(0, R), 16))
        return 1;
    icp_prepare_launch((hipStream_t)stream, R, target, origin, ref_order, icp_scratch_layout(scratch, 0, R));
    return 0;
}

extern "C" int gs2m_icp_step(int N, const double* source, const int32_t* query_order, const double* transform, int R,
                             const double* target, const double* origin, double max_dist, void* scratch, int64_t scratch_bytes,
                             void* sums, int32_t* out_idx, double* out_d2, gs2m_stream stream) {
    if (N < 0 || R < 0) {
        gs2m_set_error("gs2m_icp_step: N = %d, R = %d", N, R);
        return 1;
    }
    if (!(max_dist > 0.0) || !(max_dist < INFINITY)) {
        gs2m_set_error("gs2m_icp_step: max_dist = %g (must be positive and finite)", max_dist);
        return 1;
    }
    if (!transform || !origin || !sums || (N > 0 && !source) || (N > 0 && R > 0 && !target)) {
        gs2m_set_error("gs2m_icp_step: NULL transform, origin, sums, source or target with N = %d, R = %d", N, R);
        return 1;
    }
    if (N > 0 && gs2m_scratch_refused("gs2m_icp_step", "gs2m_icp_scratch_bytes", scratch, scratch_bytes, gs2m_icp_scratch_bytes(N, R), 16))
        return 1;
    IcpXform x;
    memcpy(x.t, transform, sizeof(x.t));
    memcpy(x.o, origin, sizeof(x.o));
    icp_step_launch((hipStream_t)stream, N, source, query_order, x, R, target, max_dist * max_dist, icp_scratch_layout(scratch, N, R),
                    (double*)sums, out_idx, out_d2);
    return 0;
}

extern "C" int gs2m_voxel_mean(int N, const double* points, const int32_t* order, int S, const int32_t* heads, double* means,
                               gs2m_stream stream) {
    if (N < 0 || S < 0) {
        gs2m_set_error("gs2m_voxel_mean: N = %d, S = %d", N, S);
        return 1;
    }
    if (S == 0) return 0;
    if (!heads || !means || (N > 0 && (!points || !order))) {
        gs2m_set_error("gs2m_voxel_mean: NULL points, order, heads or means with N = %d, S = %d", N, S);
        return 1;
    }
    GS2M_LAUNCH(k_voxel_mean, dim3(((unsigned)S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, N, points, order, S, heads, means);
    return 0;
}

extern "C" int gs2m_points_cull_views(int V, const float* points, int n_views, const float* proj, const uint64_t* mask_bits,
                                      int mask_width, int mask_height, float norm_w, float norm_h, uint8_t* keep,
                                      gs2m_stream stream) {
    if (V < 0 || n_views < 0) {
        gs2m_set_error("gs2m_points_cull_views: V = %d, n_views = %d", V, n_views);
        return 1;
    }
    if (V == 0) return 0;
    if (!points || !keep) {
        gs2m_set_error("gs2m_points_cull_views: NULL points or keep with V = %d", V);
        return 1;
    }
    if (n_views > 0) {
        if (!proj || !mask_bits) {
            gs2m_set_error("gs2m_points_cull_views: NULL proj or mask_bits with n_views = %d", n_views);
            return 1;
        }
        if (mask_width < 1 || mask_height < 1 || mask_width > (1 << 24) || mask_height > (1 << 24)) {
            gs2m_set_error("gs2m_points_cull_views: masks of %d x %d (each 1 .. 2^24)", mask_width, mask_height);
            return 1;
        }
    }
    GS2M_LAUNCH(k_points_cull_views, dim3(((unsigned)V + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, V, points, n_views, proj,
                (const unsigned long long*)mask_bits, mask_width, mask_height, (mask_width + 63) / 64, norm_w, norm_h, keep);
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
    // not gs2m_scratch_refused: one message ("state of ..., 8-byte aligned") covers the size and the alignment here
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
