// icp_kernels.h -- gs2m_icp_prepare / gs2m_icp_step: one iteration of point-to-point ICP between two f64 point sets, and
// gs2m_voxel_mean: the accumulation of Open3D's PointCloud::VoxelDownSample.  The reference aligns a prediction to the ground
// truth with Open3D's registration_icp before it scores MobileBrick (evaluation/MobileBrick/eval_code/evaluate.py:82-93) and
// TNT (evaluation/TNT/eval_code/python_toolbox/evaluation/registration.py:127-195), on host cores through a KD tree; the
// iteration is: transform the source, find every point's nearest target, keep the pairs under a threshold, and reduce them to
// the moments the closed-form (Umeyama) update needs.  include/gs2mesh_amd.h states the arithmetic; this header the layout.
//
// Prepare (once per registration).  k_icp_front writes f32(target - origin), the subtraction in f64, then pass 1 of
// knn_kernels.h (k_knn_gather / k_knn_super, nan_as_inf = 0) builds the records, boxes and super-boxes in the caller's scratch:
// exactly what gs2m_nn_dist2 builds per call.  They stay valid until the scratch is written by someone else.
//
// Step (once per iteration), three kernels on the stream, no host wait:
//   k_icp_search  p = T * s in f64, query f32(p - origin), the walk of nn_kernels.h (nn_search_wave: the same function
//                 k_nn_search calls) -> idx[i], indexed like the source.  Waves take 64 consecutive entries of `query_order`.
//   k_icp_reduce  by ORIGINAL index, so that the sums do not depend on `query_order`: recompute p (the same operations: the same
//                 bits), q = target[idx], d2 = |p - q|^2 in f64, keep iff idx >= 0 and d2 < max_dist^2, accumulate.
//   k_icp_final   adds the workgroup partials.
//
// Keep rule.  Strict `<`, as Open3D's KDTreeFlann::SearchHybrid (a radius search that drops what is not inside the radius) is
// remembered to do it: that reading is FROM MEMORY of Open3D's source, which was not at hand when this was written.
//
// Reduction tree (tests/icp_statement.py repeats it in numpy).  Every value is an f64 sum, the pair count an integer sum.
// With ICP_THREADS = 256, ICP_PER_THREAD = 4, ICP_CHUNK = 1024:
//   1. thread t of workgroup b starts from +0 and adds the terms of the kept pairs among the source indices
//      i = b * 1024 + t + 256 * k, k = 0, 1, 2, 3, in that order (acc = acc + term); a pair that is not kept adds nothing;
//   2. in a wave (lanes = 64 consecutive threads) six rounds m = 32, 16, 8, 4, 2, 1 of v = v + v[lane ^ m]: IEEE addition is
//      commutative, so both lanes of a pair hold the same bits and lane 0 ends with the pairwise tree
//      a = v[0:32] + v[32:64], a = a[0:16] + a[16:32], ..., a[0] + a[1];
//   3. across the four waves: ((w0 + w1) + w2) + w3 -> the workgroup's partial;
//   4. k_icp_final, one workgroup of 256 threads: thread t starts from +0 and adds the partials t, t + 256, t + 512, ... in that
//      order, then steps 2 and 3 again -> the sums.
// No float atomics anywhere: the same bits on every run, whatever the launch overlaps with.
//
// gs2m_voxel_mean: one thread per segment, the segment's rows added in the order given (the host side sorts stably by voxel
// key, so this is ascending original index, the order in which Open3D's AccumulatedPoint adds them), then one division per
// axis.  The sum of one segment may not be split (the bits depend on the order), so a wave per segment could only share the
// loads, not the additions; the segments of a voxel grid are short (a handful of 24-byte rows) and neighbouring segments are
// neighbours in `order`, so a thread per segment it is.  BASELINE.md has the measurement.
#pragma once
#include "nn_kernels.h"

#define ICP_SUMS 18                 // n, sum d2, sum p'[3], sum q'[3], sum p' q'^T [9], sum |p'|^2
#define ICP_THREADS 256
#define ICP_PER_THREAD 4
#define ICP_CHUNK (ICP_THREADS * ICP_PER_THREAD)

struct IcpXform {
    double t[12];                   // rows 0..2 of the row-major 4 x 4 transform
    double o[3];                    // origin
};

struct IcpScratch {
    KnnScratch knn;                 // records, boxes, super-boxes of f32(target - origin)
    float* coords;                  // [R][3] f32(target - origin): the input of k_knn_gather
    int* idx;                       // [N]: used when the caller does not ask for the indices
    double* partials;               // [blocks][ICP_SUMS]
    int blocks;
    int64_t bytes;
};

static inline IcpScratch icp_scratch_layout(void* base, int N, int R) {
    IcpScratch s;
    if (N < 0) N = 0;
    if (R < 0) R = 0;
    s.knn = knn_scratch_layout(base, R);
    if (R == 0) s.knn.bytes = 0, s.knn.groups = 0, s.knn.supers = 0;
    char* p = (char*)base + s.knn.bytes;
    s.coords = (float*)p;
    p += ((int64_t)12 * R + 15) / 16 * 16;
    s.idx = (int*)p;
    p += ((int64_t)4 * N + 15) / 16 * 16;
    s.partials = (double*)p;
    s.blocks = (int)(((int64_t)N + ICP_CHUNK - 1) / ICP_CHUNK);
    p += (int64_t)s.blocks * ICP_SUMS * 8;
    s.bytes = (int64_t)(p - (char*)base);
    return s;
}

GS2M_KERNEL void __launch_bounds__(256)
k_icp_front(int R, const double* __restrict__ target, double ox, double oy, double oz, float* __restrict__ coords) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    coords[3 * i] = (float)(target[3 * i] - ox);
    coords[3 * i + 1] = (float)(target[3 * i + 1] - oy);
    coords[3 * i + 2] = (float)(target[3 * i + 2] - oz);
}

// p = T * s, row k: ((t[k][0] * x + t[k][1] * y) + t[k][2] * z) + t[k][3]
GS2M_DEVICE void icp_transform(const IcpXform& x, const double* __restrict__ s, double p[3]) {
    const double sx = s[0], sy = s[1], sz = s[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ((x.t[4 * k] * sx + x.t[4 * k + 1] * sy) + x.t[4 * k + 2] * sz) + x.t[4 * k + 3];
}

GS2M_KERNEL void __launch_bounds__(64 * KNN_WAVES)
k_icp_search(int N, const double* __restrict__ source, const int* __restrict__ query_order, IcpXform x, int R, int groups, int supers,
             const float4* __restrict__ rec, const float4* __restrict__ box, const float4* __restrict__ sbox, int* __restrict__ out_idx) {
    __shared__ float4 tiles[KNN_WAVES][KNN_GROUP];
    const int lane = gs2m_lane(), wave = (int)(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * KNN_WAVES + wave) * 64;
    if (q0 >= N) return;                                              // whole wave: no collective is left half-attended
    const int64_t pos = q0 + lane < N ? q0 + lane : (int64_t)N - 1;
    const bool stored = q0 + lane < N;
    int id = query_order ? query_order[pos] : (int)pos;
    if ((unsigned)id >= (unsigned)N) id = (int)pos;
    double p[3];
    icp_transform(x, source + 3 * (size_t)id, p);
    const float px = (float)(p[0] - x.o[0]), py = (float)(p[1] - x.o[1]), pz = (float)(p[2] - x.o[2]);
    const bool live = stored && px == px && py == py && pz == pz;
    const unsigned long long best = nn_search_wave(px, py, pz, live, tiles[wave], R, groups, supers, rec, box, sbox);
    if (stored) out_idx[id] = (int)(unsigned)best;
}

// steps 2 and 3 of the tree; every thread of the workgroup calls it, thread 0 writes out[ICP_SUMS] (out[0] holds the integer)
GS2M_DEVICE void icp_block_reduce(long long n, double v[ICP_SUMS - 1], double (*red)[ICP_SUMS], double* __restrict__ out) {
    for (int m = 32; m >= 1; m >>= 1) {
        n = n + gs2m_shfl_xor(n, m);
#pragma unroll
        for (int a = 0; a < ICP_SUMS - 1; ++a) v[a] = v[a] + gs2m_shfl_xor(v[a], m);
    }
    const int t = (int)threadIdx.x, w = t >> 6;
    if ((t & 63) == 0) {
        ((long long*)red[w])[0] = n;
#pragma unroll
        for (int a = 0; a < ICP_SUMS - 1; ++a) red[w][1 + a] = v[a];
    }
    __syncthreads();
    if (t == 0) {
        for (int u = 1; u < ICP_THREADS / 64; ++u) {
            n = n + ((const long long*)red[u])[0];
#pragma unroll
            for (int a = 0; a < ICP_SUMS - 1; ++a) v[a] = v[a] + red[u][1 + a];
        }
        ((long long*)out)[0] = n;
#pragma unroll
        for (int a = 0; a < ICP_SUMS - 1; ++a) out[1 + a] = v[a];
    }
}

GS2M_KERNEL void __launch_bounds__(ICP_THREADS)
k_icp_reduce(int N, const double* __restrict__ source, IcpXform x, int R, const double* __restrict__ target,
             const int* __restrict__ idx, double max2, double* __restrict__ partials, double* __restrict__ out_d2) {
    __shared__ double red[ICP_THREADS / 64][ICP_SUMS];
    long long n = 0;
    double v[ICP_SUMS - 1];
#pragma unroll
    for (int a = 0; a < ICP_SUMS - 1; ++a) v[a] = 0.0;
    for (int k = 0; k < ICP_PER_THREAD; ++k) {
        const int64_t i = (int64_t)blockIdx.x * ICP_CHUNK + (int64_t)k * ICP_THREADS + threadIdx.x;
        if (i >= N) break;
        const int j = idx[i];
        double d2 = INFINITY;
        if ((unsigned)j < (unsigned)R) {                              // -1 = no neighbour; anything else out of range = a scratch nobody prepared
            double p[3];
            icp_transform(x, source + 3 * (size_t)i, p);
            const double* q = target + 3 * (size_t)j;
            const double qx = q[0], qy = q[1], qz = q[2];
            const double dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
            d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < max2) {
                const double ax = p[0] - x.o[0], ay = p[1] - x.o[1], az = p[2] - x.o[2];
                const double bx = qx - x.o[0], by = qy - x.o[1], bz = qz - x.o[2];
                n = n + 1;
                v[0] = v[0] + d2;
                v[1] = v[1] + ax, v[2] = v[2] + ay, v[3] = v[3] + az;
                v[4] = v[4] + bx, v[5] = v[5] + by, v[6] = v[6] + bz;
                v[7] = v[7] + ax * bx, v[8] = v[8] + ax * by, v[9] = v[9] + ax * bz;
                v[10] = v[10] + ay * bx, v[11] = v[11] + ay * by, v[12] = v[12] + ay * bz;
                v[13] = v[13] + az * bx, v[14] = v[14] + az * by, v[15] = v[15] + az * bz;
                v[16] = v[16] + ((ax * ax + ay * ay) + az * az);
            }
        }
        if (out_d2) out_d2[i] = d2;
    }
    icp_block_reduce(n, v, red, partials + (size_t)blockIdx.x * ICP_SUMS);
}

GS2M_KERNEL void __launch_bounds__(ICP_THREADS)
k_icp_final(int blocks, const double* __restrict__ partials, double* __restrict__ sums) {
    __shared__ double red[ICP_THREADS / 64][ICP_SUMS];
    long long n = 0;
    double v[ICP_SUMS - 1];
#pragma unroll
    for (int a = 0; a < ICP_SUMS - 1; ++a) v[a] = 0.0;
    for (int b = (int)threadIdx.x; b < blocks; b += ICP_THREADS) {
        const double* p = partials + (size_t)b * ICP_SUMS;
        n = n + ((const long long*)p)[0];
#pragma unroll
        for (int a = 0; a < ICP_SUMS - 1; ++a) v[a] = v[a] + p[1 + a];
    }
    icp_block_reduce(n, v, red, sums);
}

static void icp_prepare_launch(hipStream_t stream, int R, const double* target, const double* origin, const int* ref_order,
                               const IcpScratch& s) {
    GS2M_LAUNCH(k_icp_front, dim3(((unsigned)R + 255u) / 256u), dim3(256), 0, stream, R, target, origin[0], origin[1], origin[2],
                s.coords);
    GS2M_LAUNCH(k_knn_gather, dim3((unsigned)s.knn.groups), dim3(KNN_GROUP), 0, stream, R, (const float*)s.coords, ref_order, 0,
                s.knn.rec, s.knn.box);
    GS2M_LAUNCH(k_knn_super, dim3((unsigned)((s.knn.supers + 63) / 64)), dim3(64), 0, stream, s.knn.groups, s.knn.supers,
                (const float4*)s.knn.box, s.knn.sbox);
}

static void icp_step_launch(hipStream_t stream, int N, const double* source, const int* query_order, const IcpXform& x, int R,
                            const double* target, double max2, const IcpScratch& s, double* sums, int* out_idx, double* out_d2) {
    if (N > 0) {
        int* idx = out_idx ? out_idx : s.idx;
        const unsigned blocks = (unsigned)(((int64_t)N + 64 * KNN_WAVES - 1) / (64 * KNN_WAVES));
        GS2M_LAUNCH(k_icp_search, dim3(blocks), dim3(64 * KNN_WAVES), 0, stream, N, source, query_order, x, R, s.knn.groups,
                    s.knn.supers, (const float4*)s.knn.rec, (const float4*)s.knn.box, (const float4*)s.knn.sbox, idx);
        GS2M_LAUNCH(k_icp_reduce, dim3((unsigned)s.blocks), dim3(ICP_THREADS), 0, stream, N, source, x, R, target, (const int*)idx,
                    max2, s.partials, out_d2);
    }
    GS2M_LAUNCH(k_icp_final, dim3(1), dim3(ICP_THREADS), 0, stream, N > 0 ? s.blocks : 0, (const double*)s.partials, sums);
}

// ---- gs2m_voxel_mean -------------------------------------------------------------------------------------------------------

// An `order` entry outside [0, N) or a head outside [0, N] (the caller broke the precondition) is clamped, so nothing is
// read out of bounds.  An empty segment gives 0 / 0 = NaN.
GS2M_KERNEL void __launch_bounds__(256)
k_voxel_mean(int N, const double* __restrict__ points, const int* __restrict__ order, int S, const int* __restrict__ heads,
             double* __restrict__ means) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int b = heads[s], e = s + 1 < S ? heads[s + 1] : N;
    b = b < 0 ? 0 : (b > N ? N : b);
    e = e < b ? b : (e > N ? N : e);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = b; k < e; ++k) {
        int id = order[k];
        if ((unsigned)id >= (unsigned)N) id = k;
        sx = sx + points[3 * (size_t)id], sy = sy + points[3 * (size_t)id + 1], sz = sz + points[3 * (size_t)id + 2];
    }
    const double c = (double)(e - b);
    means[3 * s] = sx / c, means[3 * s + 1] = sy / c, means[3 * s + 2] = sz / c;
}
