// nn_kernels.h -- gs2m_nn_dist2: for every query point its nearest neighbour in ANOTHER point set, squared distance and
// index, the hot path of every geometric mesh metric (DTU accuracy / completeness, MobileBrick accuracy / recall / F1,
// the TNT F-score: evaluation/DTU/eval_code/eval.py:119-134, evaluation/MobileBrick/eval_code/evaluate.py:46-63, which run
// it on host cores through KD and ball trees).
//
// Arithmetic and selection (include/gs2mesh_amd.h states them): d = (dx*dx + dy*dy) + dz*dz in f32 without contraction,
// the best is the minimum of (d, j) in lexicographic order over all references j whose d is not NaN.  The minimum of a set
// does not depend on the order in which it is walked, so the result is a function of the two point sets alone.
//
// The best is carried as ONE u64 key, (bits(d) << 32) | j: d is +0 or larger (a sum of squares), so the f32 bit patterns
// order like the values; +inf is 0x7f800000 and every NaN pattern, of either sign, is larger.  The walk starts from
// (bits(+inf), 0xffffffff) = (+inf, none): a candidate at d = +inf has a smaller key and replaces it (its j < 2^31), a NaN
// has a larger key and never does, and the low word read as int32 is -1 while nothing has replaced it.
//
// Layout.  The references go through pass 1 of knn_kernels.h with nan_as_inf = 0 (k_knn_gather, k_knn_super: 16-byte records in
// `ref_order`, a box per 256 records, a super-box per 16 boxes).  Pass 2 gives every wave 64 consecutive queries of
// `query_order`, one per lane.  A query has no group of its own, so the wave first looks for a place to start: the lanes
// share out ALL super-boxes (R / 4096 of them), each takes the distance between a super-box and the box of the wave's
// queries, and a wave arg-min picks the nearest; inside it lanes 0..15 do the same over its groups.  From there the walk
// goes outwards as in the kNN: with both sets along a space-filling curve index distance tracks spatial distance, so the
// bound is near its final value after the first group.  Any start is correct, only the time depends on it.
//
// Culling is knn_box_dist2, exact in f32 by the argument of knn_kernels.h: box distance <= d of every point in the box.
// A group is skipped only when its box distance is > the lane's best d in every live lane (wave-uniform, and STRICT: a box
// at a distance equal to the best may hold a smaller index at that same distance, which must win).  Lanes that did not
// need a staged group compare its candidates anyway; every one of them is farther than their best and changes nothing.
// Coordinates that are NaN never enter a box (k_knn_gather leaves them out), so a reference with a NaN
// coordinate may sit in a box that does not contain it: its d is NaN and it is never selected, wherever it is met.
// A query with a NaN coordinate has d = NaN to everything; it asks for no group and keeps (+inf, none).
#pragma once
#include "knn_kernels.h"

#define NN_NONE 0x7f800000ffffffffull       // (+inf, no index)

GS2M_DEVICE unsigned long long nn_key(float d, float index_bits) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(index_bits);
}
GS2M_DEVICE unsigned long long nn_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

// distance between two boxes, in the form of knn_box_dist2; only ranks the places to start at
GS2M_DEVICE float nn_box_box_dist2(const float lo[3], const float hi[3], const float4 mn, const float4 mx) {
    const float dx = fmaxf(fmaxf(mn.x - hi[0], lo[0] - mx.x), 0.0f);
    const float dy = fmaxf(fmaxf(mn.y - hi[1], lo[1] - mx.y), 0.0f);
    const float dz = fmaxf(fmaxf(mn.z - hi[2], lo[2] - mx.z), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

// The walk of one wave: lane l's query is (px, py, pz), `live` where the lane has a query without a NaN coordinate (a NaN query
// asks for nothing and finds nothing); -> the lane's best key.  Called by every lane of the wave (it holds wave collectives);
// `tile` is the wave's own KNN_GROUP records of LDS.  The one walk of the library: k_nn_search and the ICP step
// (icp_kernels.h), which differ only in where a query comes from, both call it.
GS2M_DEVICE unsigned long long nn_search_wave(float px, float py, float pz, bool live, float4* tile, int R, int groups, int supers,
                                              const float4* __restrict__ rec, const float4* __restrict__ box,
                                              const float4* __restrict__ sbox) {
    const int lane = gs2m_lane();
    unsigned long long best = NN_NONE;
    if (supers > 0) {
        // the box of the wave's queries, then the nearest super-box and the nearest group in it
        float lo[3] = {live ? px : INFINITY, live ? py : INFINITY, live ? pz : INFINITY};
        float hi[3] = {live ? px : -INFINITY, live ? py : -INFINITY, live ? pz : -INFINITY};
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int m = 32; m >= 1; m >>= 1) {
                lo[a] = fminf(lo[a], gs2m_shfl_xor(lo[a], m));
                hi[a] = fmaxf(hi[a], gs2m_shfl_xor(hi[a], m));
            }
        unsigned long long near = ~0ull;
        for (int s = lane; s < supers; s += 64)
            near = nn_min(near, ((unsigned long long)__float_as_uint(nn_box_box_dist2(lo, hi, sbox[2 * (size_t)s], sbox[2 * (size_t)s + 1])) << 32) |
                                    (unsigned)s);
        for (int m = 32; m >= 1; m >>= 1) near = nn_min(near, gs2m_shfl_xor(near, m));
        int s_start = (int)(unsigned)near;
        s_start = gs2m_uniform((unsigned)s_start < (unsigned)supers ? s_start : 0);
        const int f_lo = s_start * KNN_FAN;
        near = ~0ull;
        if (lane < KNN_FAN && f_lo + lane < groups)
            near = ((unsigned long long)__float_as_uint(nn_box_box_dist2(lo, hi, box[2 * (size_t)(f_lo + lane)], box[2 * (size_t)(f_lo + lane) + 1])) << 32) |
                   (unsigned)(f_lo + lane);
        for (int m = 32; m >= 1; m >>= 1) near = nn_min(near, gs2m_shfl_xor(near, m));
        int g_start = (int)(unsigned)near;
        g_start = gs2m_uniform((unsigned)g_start < (unsigned)groups ? g_start : f_lo);

        const int s_steps = 2 * (s_start > supers - 1 - s_start ? s_start : supers - 1 - s_start) + 1;
        for (int ts = 0; ts < s_steps; ++ts) {
            const int s = knn_outward(s_start, ts);
            if (s < 0 || s >= supers) continue;
            if (gs2m_ballot_b(live && !(knn_box_dist2(px, py, pz, sbox[2 * (size_t)s], sbox[2 * (size_t)s + 1]) > __uint_as_float((unsigned)(best >> 32)))) == 0ull)
                continue;
            const int c_lo = s * KNN_FAN, c_hi = (c_lo + KNN_FAN < groups ? c_lo + KNN_FAN : groups) - 1;
            const int centre = g_start < c_lo ? c_lo : (g_start > c_hi ? c_hi : g_start);
            const int c_steps = 2 * (centre - c_lo > c_hi - centre ? centre - c_lo : c_hi - centre) + 1;
            for (int tc = 0; tc < c_steps; ++tc) {
                const int c = knn_outward(centre, tc);
                if (c < c_lo || c > c_hi) continue;
                if (gs2m_ballot_b(live && !(knn_box_dist2(px, py, pz, box[2 * (size_t)c], box[2 * (size_t)c + 1]) > __uint_as_float((unsigned)(best >> 32)))) == 0ull)
                    continue;
                const int64_t base = (int64_t)c * KNN_GROUP;
                const int n = R - base < KNN_GROUP ? (int)(R - base) : KNN_GROUP;
                gs2m_wave_sync();                                     // every lane is done with the tile's last content
#pragma unroll
                for (int k = 0; k < KNN_GROUP / 64; ++k)
                    if (lane + 64 * k < n) tile[lane + 64 * k] = rec[base + lane + 64 * k];
                gs2m_wave_sync();
#pragma unroll 8
                for (int j = 0; j < n; ++j) {
                    const float4 q = tile[j];
                    best = nn_min(best, nn_key(knn_dist2(px, py, pz, q.x, q.y, q.z), q.w));
                }
            }
        }
    }
    return best;
}

// Pass 2.  Waves are independent (no workgroup barrier): KNN_WAVES of them share a workgroup only to fill a CU.
// groups = supers = 0 (no references) writes (+inf, -1).
GS2M_KERNEL void __launch_bounds__(64 * KNN_WAVES)
k_nn_search(int Q, const float* __restrict__ queries, const int* __restrict__ query_order, int R, int groups, int supers,
            const float4* __restrict__ rec, const float4* __restrict__ box, const float4* __restrict__ sbox,
            float* __restrict__ out_d2, int* __restrict__ out_idx) {
    __shared__ float4 tiles[KNN_WAVES][KNN_GROUP];
    const int lane = gs2m_lane(), wave = (int)(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * KNN_WAVES + wave) * 64;
    if (q0 >= Q) return;                                              // whole wave: no collective is left half-attended
    const int64_t pos = q0 + lane < Q ? q0 + lane : (int64_t)Q - 1;
    const bool stored = q0 + lane < Q;
    int id = query_order ? query_order[pos] : (int)pos;
    if ((unsigned)id >= (unsigned)Q) id = (int)pos;
    const float px = queries[3 * (size_t)id], py = queries[3 * (size_t)id + 1], pz = queries[3 * (size_t)id + 2];
    const bool live = stored && px == px && py == py && pz == pz;   // a NaN query asks for nothing and finds nothing
    const unsigned long long best = nn_search_wave(px, py, pz, live, tiles[wave], R, groups, supers, rec, box, sbox);
    if (stored) {
        out_d2[id] = __uint_as_float((unsigned)(best >> 32));
        if (out_idx) out_idx[id] = (int)(unsigned)best;
    }
}

static void nn_launch(hipStream_t stream, int Q, const float* queries, const int* query_order, int R, const float* refs,
                      const int* ref_order, const KnnScratch& s, float* out_d2, int* out_idx) {
    if (R > 0) {
        GS2M_LAUNCH(k_knn_gather, dim3((unsigned)s.groups), dim3(KNN_GROUP), 0, stream, R, refs, ref_order, 0, s.rec, s.box);
        GS2M_LAUNCH(k_knn_super, dim3((unsigned)((s.supers + 63) / 64)), dim3(64), 0, stream, s.groups, s.supers,
                    (const float4*)s.box, s.sbox);
    }
    const unsigned blocks = (unsigned)(((int64_t)Q + 64 * KNN_WAVES - 1) / (64 * KNN_WAVES));
    GS2M_LAUNCH(k_nn_search, dim3(blocks), dim3(64 * KNN_WAVES), 0, stream, Q, queries, query_order, R, R > 0 ? s.groups : 0,
                R > 0 ? s.supers : 0, (const float4*)s.rec, (const float4*)s.box, (const float4*)s.sbox, out_d2, out_idx);
}
