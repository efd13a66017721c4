// knn_kernels.h -- gs2m_knn_mean_dist2: for every point the mean of the three smallest squared distances to the other
// points, the one native kernel 3DGS training needs besides the rasteriser (simple-knn's distCUDA2,
// submodules/simple-knn/simple_knn.cu:131-183; GaussianModel.create_from_pcd turns it into the initial scales).
//
// Arithmetic (include/gs2mesh_amd.h states it): d = (dx*dx + dy*dy) + dz*dz in f32 without contraction (this header is
// compiled into points_kernels.hip, built with -ffp-contract=off), the three smallest d over all OTHER points, missing
// ones FLT_MAX, out = ((b0 + b1) + b2) / 3.  The three smallest values of a multiset do not depend on the order in
// which it is walked, so the result is a function of the point set alone: not of `order`, not of the launch shape.
//
// Input that is not finite: the reference's rule (updateKBest, :132-145).  A candidate counts only if its d is below the
// current third best, which starts at FLT_MAX; so a d that is NaN or not below FLT_MAX never counts, and the triple is
// the three smallest counting d, padded with FLT_MAX.  A point with a NaN or infinite coordinate therefore gets +inf
// ((FLT_MAX + FLT_MAX) + FLT_MAX; not NaN, not an error) and changes no other point's result, and a neighbour so far
// away that d overflows is a neighbour at "no distance": it stands as FLT_MAX, like a missing one.  How the kernel keeps
// that rule without a test per candidate is said at k_knn_search.
//
// Layout.  Pass 1 gathers the points in `order` into 16-byte records (x, y, z, caller's index) and writes one box per
// GROUP of KNN_GROUP consecutive records; a second small kernel joins KNN_FAN boxes into a super-box.  Pass 2 gives
// every wave 64 consecutive records as its queries, one per lane, and walks the super-boxes outwards from its own
// (the order is along a space-filling curve when the caller sorted: near groups come first and the bound drops fast),
// inside a super-box the groups outwards from the nearest one.  A group is staged into the wave's own LDS tile with
// coalesced 16-byte loads and then read by every lane as a broadcast (one ds_read_b128 per candidate per wave, no
// per-candidate gather from global memory as in the reference, :175-180).
//
// Culling is exact in f32.  For a box [mn, mx] and a query p the per-axis gap is max(mn - p, p - mx, 0): when p is
// outside this is the reference's min(|p - mn|, |p - mx|) (:119-129; fl(a - b) = -fl(b - a)), and for any q in the box
// |fl(q - p)| >= gap because rounding is monotone; squaring and the two additions, written in the form of the point
// distance, are monotone too.  So box distance <= distance of every point in the box, a group whose box distance
// is > the lane's third-best can hold nothing that would change it (strict: a tie is still visited, and would not change
// the values either), and a super-box contains its boxes, so its distance is <= theirs.  The skip is wave-uniform: a
// group is skipped only if no lane of the wave needs it; lanes that did not need it compare its candidates anyway, which
// changes nothing because every candidate is >= the box distance > that lane's third-best.
#pragma once
#include <float.h>

#define KNN_GROUP 256          // records per box = candidates per staged tile (4 KiB of LDS per wave)
#define KNN_FAN 16             // boxes per super-box
#define KNN_WAVES 4            // waves (of 64 queries) per workgroup of pass 2

struct KnnScratch {
    float4* rec;               // [P] x, y, z, bits of the caller's index
    float4* box;               // [2 * groups] min, max
    float4* sbox;              // [2 * supers]
    int groups, supers;
    int64_t bytes;
};

static inline KnnScratch knn_scratch_layout(void* base, int P) {
    KnnScratch s;
    s.groups = (int)(((int64_t)P + KNN_GROUP - 1) / KNN_GROUP);
    s.supers = (s.groups + KNN_FAN - 1) / KNN_FAN;
    s.rec = (float4*)base;
    s.box = s.rec + (size_t)P;
    s.sbox = s.box + 2 * (size_t)s.groups;
    s.bytes = 16 * ((int64_t)P + 2 * (int64_t)s.groups + 2 * (int64_t)s.supers);
    return s;
}

// insert d into the ascending triple: the new k-th value is the median of the old (k-1)-th, k-th and d.  v_med3_f32
// with a NaN operand returns the minimum of the others; the emulator's form has the same rule, so both back-ends run
// the same function.  A NaN d would thus turn (b0, b1, b2) into (b0, b0, b1): knn_insert must never see one while
// the triple holds anything below FLT_MAX (k_knn_search says why it does not).
#ifdef __HIPCC__
GS2M_DEVICE float knn_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
#else
GS2M_DEVICE float knn_med3(float a, float b, float c) {
    if (a != a || b != b || c != c) return fminf(fminf(a, b), c);
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}
#endif
GS2M_DEVICE void knn_insert(float& b0, float& b1, float& b2, float d) {
    b2 = knn_med3(b1, b2, d);
    b1 = knn_med3(b0, b1, d);
    b0 = fminf(b0, d);
}

GS2M_DEVICE float knn_dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

GS2M_DEVICE float knn_box_dist2(float px, float py, float pz, const float4 mn, const float4 mx) {
    const float dx = fmaxf(fmaxf(mn.x - px, px - mx.x), 0.0f);
    const float dy = fmaxf(fmaxf(mn.y - py, py - mx.y), 0.0f);
    const float dz = fmaxf(fmaxf(mn.z - pz, pz - mx.z), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

// Pass 1: one workgroup per group.  An `order` entry outside [0, P) (the caller broke the precondition) is replaced by the
// position, so nothing is ever read or written out of bounds.  A NaN coordinate never enters a box.  With nan_as_inf
// (the kNN; gs2m_nn_dist2 keeps the NaN, which its key never selects) it is stored as +inf in the record.
GS2M_KERNEL void __launch_bounds__(KNN_GROUP)
k_knn_gather(int P, const float* __restrict__ points, const int* __restrict__ order, int nan_as_inf, float4* __restrict__ rec,
             float4* __restrict__ box) {
    __shared__ float red[2 * 3 * (KNN_GROUP / 64)];
    const int t = (int)threadIdx.x, g = (int)blockIdx.x;
    const int64_t pos = (int64_t)g * KNN_GROUP + t;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (pos < P) {
        int id = order ? order[pos] : (int)pos;
        if ((unsigned)id >= (unsigned)P) id = (int)pos;
        const float x = points[3 * (size_t)id], y = points[3 * (size_t)id + 1], z = points[3 * (size_t)id + 2];
        rec[pos] = make_float4(nan_as_inf && x != x ? INFINITY : x, nan_as_inf && y != y ? INFINITY : y,
                               nan_as_inf && z != z ? INFINITY : z, __int_as_float(id));
        if (x == x) lo[0] = hi[0] = x;
        if (y == y) lo[1] = hi[1] = y;
        if (z == z) lo[2] = hi[2] = z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int m = 32; m >= 1; m >>= 1) {
            lo[a] = fminf(lo[a], gs2m_shfl_xor(lo[a], m));
            hi[a] = fmaxf(hi[a], gs2m_shfl_xor(hi[a], m));
        }
    const int w = t >> 6;
    if ((t & 63) == 0)
        for (int a = 0; a < 3; ++a) {
            red[6 * w + a] = lo[a];
            red[6 * w + 3 + a] = hi[a];
        }
    __syncthreads();
    if (t == 0) {
        for (int v = 1; v < KNN_GROUP / 64; ++v)
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], red[6 * v + a]);
                hi[a] = fmaxf(hi[a], red[6 * v + 3 + a]);
            }
        box[2 * (size_t)g] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        box[2 * (size_t)g + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

GS2M_KERNEL void __launch_bounds__(64)
k_knn_super(int groups, int supers, const float4* __restrict__ box, float4* __restrict__ sbox) {
    const int s = (int)(blockIdx.x * 64u + threadIdx.x);
    if (s >= supers) return;
    const int b0 = s * KNN_FAN, b1 = b0 + KNN_FAN < groups ? b0 + KNN_FAN : groups;
    float4 lo = box[2 * (size_t)b0], hi = box[2 * (size_t)b0 + 1];
    for (int b = b0 + 1; b < b1; ++b) {
        const float4 l = box[2 * (size_t)b], h = box[2 * (size_t)b + 1];
        lo.x = fminf(lo.x, l.x), lo.y = fminf(lo.y, l.y), lo.z = fminf(lo.z, l.z);
        hi.x = fmaxf(hi.x, h.x), hi.y = fmaxf(hi.y, h.y), hi.z = fmaxf(hi.z, h.z);
    }
    sbox[2 * (size_t)s] = lo;
    sbox[2 * (size_t)s + 1] = hi;
}

// the t-th index of the walk outwards from `centre`: centre, centre + 1, centre - 1, centre + 2, ...
GS2M_DEVICE int knn_outward(int centre, int t) { return (t & 1) ? centre + ((t + 1) >> 1) : centre - (t >> 1); }

// Pass 2.  Waves are independent (no workgroup barrier): KNN_WAVES of them share a workgroup only to fill a CU.
// Non-finite input costs nothing per candidate.  Pass 1 stored every NaN coordinate as +inf, so a record's coordinates are
// finite or infinite.  A query with finite coordinates then gets d = +inf from a record with an infinite one (finite - inf
// squares to +inf, and a sum of squares has no inf - inf) and never a NaN; med3 and min drop a +inf because the triple
// never exceeds FLT_MAX.  A query with an infinite coordinate gets +inf or NaN (inf - inf) from every record, and its triple
// is still (FLT_MAX, FLT_MAX, FLT_MAX) whenever a NaN arrives: med3(FLT_MAX, FLT_MAX, NaN) = FLT_MAX under either rule.
GS2M_KERNEL void __launch_bounds__(64 * KNN_WAVES)
k_knn_search(int P, int groups, int supers, const float4* __restrict__ rec, const float4* __restrict__ box,
             const float4* __restrict__ sbox, float* __restrict__ out) {
    __shared__ float4 tiles[KNN_WAVES][KNN_GROUP];
    const int lane = gs2m_lane(), wave = (int)(threadIdx.x >> 6);
    float4* tile = tiles[wave];
    const int64_t q0 = ((int64_t)blockIdx.x * KNN_WAVES + wave) * 64;
    if (q0 >= P) return;                                              // whole wave: no collective is left half-attended
    const int64_t pos = q0 + lane;
    const bool live = pos < P;
    const float4 me = rec[live ? pos : (int64_t)P - 1];
    const float px = me.x, py = me.y, pz = me.z;
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    const int g_own = (int)(q0 / KNN_GROUP), s_own = g_own / KNN_FAN;
    const int s_steps = 2 * (s_own > supers - 1 - s_own ? s_own : supers - 1 - s_own) + 1;
    for (int ts = 0; ts < s_steps; ++ts) {
        const int s = knn_outward(s_own, ts);
        if (s < 0 || s >= supers) continue;
        if (gs2m_ballot_b(live && !(knn_box_dist2(px, py, pz, sbox[2 * (size_t)s], sbox[2 * (size_t)s + 1]) > b2)) == 0ull) continue;
        const int c_lo = s * KNN_FAN, c_hi = (c_lo + KNN_FAN < groups ? c_lo + KNN_FAN : groups) - 1;
        const int centre = g_own < c_lo ? c_lo : (g_own > c_hi ? c_hi : g_own);
        const int c_steps = 2 * (centre - c_lo > c_hi - centre ? centre - c_lo : c_hi - centre) + 1;
        for (int tc = 0; tc < c_steps; ++tc) {
            const int c = knn_outward(centre, tc);
            if (c < c_lo || c > c_hi) continue;
            if (gs2m_ballot_b(live && !(knn_box_dist2(px, py, pz, box[2 * (size_t)c], box[2 * (size_t)c + 1]) > b2)) == 0ull) continue;
            const int64_t base = (int64_t)c * KNN_GROUP;
            const int n = P - base < KNN_GROUP ? (int)(P - base) : KNN_GROUP;
            gs2m_wave_sync();                                         // every lane is done with the tile's last content
#pragma unroll
            for (int k = 0; k < KNN_GROUP / 64; ++k)
                if (lane + 64 * k < n) tile[lane + 64 * k] = rec[base + lane + 64 * k];
            gs2m_wave_sync();
            if (c == g_own) {
                const int self = (int)(pos - base);                   // "other" is by index = by position in the order
#pragma unroll 4
                for (int j = 0; j < n; ++j) {
                    const float4 q = tile[j];
                    const float d = knn_dist2(px, py, pz, q.x, q.y, q.z);
                    knn_insert(b0, b1, b2, j == self ? FLT_MAX : d);
                }
            } else {
#pragma unroll 8
                for (int j = 0; j < n; ++j) {
                    const float4 q = tile[j];
                    knn_insert(b0, b1, b2, knn_dist2(px, py, pz, q.x, q.y, q.z));
                }
            }
        }
    }
    if (live) out[__float_as_int(me.w)] = ((b0 + b1) + b2) / 3.0f;
}

static void knn_launch(hipStream_t stream, int P, const float* points, const int* order, const KnnScratch& s, float* out) {
    GS2M_LAUNCH(k_knn_gather, dim3((unsigned)s.groups), dim3(KNN_GROUP), 0, stream, P, points, order, 1, s.rec, s.box);
    GS2M_LAUNCH(k_knn_super, dim3((unsigned)((s.supers + 63) / 64)), dim3(64), 0, stream, s.groups, s.supers,
                (const float4*)s.box, s.sbox);
    const unsigned blocks = (unsigned)(((int64_t)P + 64 * KNN_WAVES - 1) / (64 * KNN_WAVES));
    GS2M_LAUNCH(k_knn_search, dim3(blocks), dim3(64 * KNN_WAVES), 0, stream, P, s.groups, s.supers, (const float4*)s.rec,
                (const float4*)s.box, (const float4*)s.sbox, out);
}
