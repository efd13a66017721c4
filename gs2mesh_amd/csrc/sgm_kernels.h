// sgm_kernels.h -- gs2m_stereo_sgm: four-path semi-global matching on a 9 x 7 census, the built-in (weights-free)
// matcher of gs2mesh_amd.stereo_utils.Stereo.  Included by stereo_kernels.hip (-ffp-contract=off).
//
// Arithmetic (integer up to the sub-pixel step, so the result is defined bit for bit; include/gs2mesh_amd.h states it):
//   grey    g = (77 R + 150 G + 29 B + 128) >> 8
//   census  62 bits, bit = g(neighbour) < g(centre), 9 wide x 7 high, edge replicate
//   cost    C(y,x,d) = popcount(census_base(y,x) ^ census_other(y, x - sgn d)), 62 where x - sgn d leaves the image
//           (sgn = +1: left-based pass, base = left; sgn = -1: right-based pass, base = right)
//   path    L_r(p,d) = C(p,d) + min(L_r(p',d), L_r(p',d-1) + P1, L_r(p',d+1) + P1, m + P2) - m,  m = min_k L_r(p',k)
//   S = L_right + L_left + L_down + L_up,  d* = lowest argmin,  parabola through S(d*-1), S(d*), S(d*+1) in f32
//
// Shape.  C is never stored: a cost is one 64-bit xor + popcount of two census words (both census images stay in cache).
// One wave walks one path; its 64 lanes hold the D = 64 K disparities of the current pixel, lane l owning the K
// consecutive ones d = l K + k.  So d - 1 / d + 1 are registers of the same lane except at the two ends (one cross-lane
// move each per step), the K path costs of a lane are one contiguous K-byte (or 2K-byte) piece of a [H][W][D] plane, a wave's
// pieces are one contiguous row of D, and the minimum m is K - 1 per-lane minima plus one wave reduction.  No LDS, no
// barrier: the only thing a step waits for is the previous step of its own path.
//   k_sgm_horizontal  one wave per (row, direction): writes L_right and L_left as two u8 planes.  The census words of the
//                     other image slide through the lanes (a step needs the window of the step before, moved by one
//                     disparity), so a step loads nothing: the base word and the one new window word of the next 64
//                     steps are fetched by one coalesced load per lane, 64 steps ahead.
//   k_sgm_down        one wave per column: reads the two planes, adds its own L_down, writes the u16 plane S'.
//   k_sgm_up          one wave per column, bottom to top: S = S' + L_up is complete in registers, so the winner and the
//                     sub-pixel step happen here and S goes to memory only when the caller asks for it (tap).
//                     Both column kernels issue the loads of the next row before they work on the current one.
#pragma once

#define SGM_OOB_COST 62
#define SGM_INF (1 << 20)
#define SGM_MAX_K 16          // D <= 1024

constexpr int sgm_pow2_align(int bytes) {
    return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : bytes % 4 == 0 ? 4 : bytes % 2 == 0 ? 2 : 1;
}
// the K values of one lane in a plane: loaded / stored with the widest instruction its size allows
template <typename T, int K>
struct alignas(sgm_pow2_align(K * (int)sizeof(T))) SgmPack {
    T v[K];
};

GS2M_DEVICE int sgm_min(int a, int b) { return b < a ? b : a; }
// Cross-lane steps of a path.  They are the whole dependent chain of a step, so the product build keeps them in the
// vector ALU (data-parallel-primitive moves, a few cycles each) instead of eight trips through the LDS crossbar; min is
// idempotent, so a lane that has no source simply keeps its own value.  The emulator build takes the shuffle form.
#ifdef __HIPCC__
#define SGM_DPP(old, src, ctrl) __builtin_amdgcn_update_dpp((old), (src), (ctrl), 0xf, 0xf, false)
GS2M_DEVICE int sgm_wave_min(int v) {
    v = sgm_min(v, SGM_DPP(v, v, 0x111));     // row_shr:1, 2, 4, 8: lane 15 of every row of 16 holds the row's minimum
    v = sgm_min(v, SGM_DPP(v, v, 0x112));
    v = sgm_min(v, SGM_DPP(v, v, 0x114));
    v = sgm_min(v, SGM_DPP(v, v, 0x118));
    v = sgm_min(v, SGM_DPP(v, v, 0x142));     // row_bcast:15: lane 15 of a row into the next row
    v = sgm_min(v, SGM_DPP(v, v, 0x143));     // row_bcast:31: lane 31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}
// the value of lane - 1 / lane + 1; `edge` in lane 0 / lane 63
GS2M_DEVICE int sgm_from_lane_below(int v, int edge, int) { return SGM_DPP(edge, v, 0x138); }     // wave_shr:1
GS2M_DEVICE int sgm_from_lane_above(int v, int edge, int) { return SGM_DPP(edge, v, 0x130); }     // wave_shl:1
#else
GS2M_DEVICE int sgm_wave_min(int v) {
    for (int m = 32; m >= 1; m >>= 1) v = sgm_min(v, gs2m_shfl_xor(v, m));
    return v;
}
GS2M_DEVICE int sgm_from_lane_below(int v, int edge, int lane) {
    const int r = gs2m_shfl_up(v, 1);
    return lane == 0 ? edge : r;
}
GS2M_DEVICE int sgm_from_lane_above(int v, int edge, int lane) {
    const int r = gs2m_shfl(v, lane + 1);
    return lane == 63 ? edge : r;
}
#endif

// ---- grey + census --------------------------------------------------------------------------------------------
GS2M_KERNEL void __launch_bounds__(256)
k_sgm_grey(const unsigned char* __restrict__ rgb_l, const unsigned char* __restrict__ rgb_r, int n, unsigned char* __restrict__ grey) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const unsigned char* p = (blockIdx.y ? rgb_r : rgb_l) + (size_t)i * 3;
    grey[(size_t)blockIdx.y * n + i] = (unsigned char)((77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8);
}

GS2M_KERNEL void __launch_bounds__(256)
k_sgm_census(const unsigned char* __restrict__ grey, int W, int H, unsigned long long* __restrict__ census) {
    const int x = (int)(blockIdx.x * 256u + threadIdx.x);
    const int y = (int)blockIdx.y;
    if (x >= W) return;
    const unsigned char* g = grey + (size_t)blockIdx.z * W * H;
    const int c = g[(size_t)y * W + x];
    unsigned long long bits = 0ull;
    for (int dy = -3; dy <= 3; ++dy) {
        int yy = y + dy;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        const unsigned char* row = g + (size_t)yy * W;
        for (int dx = -4; dx <= 4; ++dx) {
            if (dy == 0 && dx == 0) continue;
            int xx = x + dx;
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            bits = (bits << 1) | (unsigned long long)((int)row[xx] < c);
        }
    }
    census[((size_t)blockIdx.z * H + y) * W + x] = bits;
}

// ---- one step of a path ---------------------------------------------------------------------------------------
// L: path costs of the previous pixel (in) / of this pixel (out); m: their minimum over all D (in / out)
template <int K>
GS2M_DEVICE void sgm_path_step(int (&L)[K], const int (&C)[K], int& m, int P1, int P2, int lane) {
    int below = sgm_from_lane_below(L[K - 1], SGM_INF, lane);       // L(d0 - 1): the last value of the lane before
    const int above = sgm_from_lane_above(L[0], SGM_INF, lane);     // L(d0 + K): the first value of the lane after
    const int jump = m + P2;
    int lane_min = SGM_INF;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int same = L[k];
        const int up = (k + 1 < K ? L[k + 1] : above) + P1;
        const int best = sgm_min(sgm_min(same, below + P1), sgm_min(up, jump));
        below = same;
        L[k] = C[k] + best - m;
        lane_min = sgm_min(lane_min, L[k]);
    }
    m = sgm_wave_min(lane_min);
}

template <int K>
GS2M_DEVICE void sgm_path_first(int (&L)[K], const int (&C)[K], int& m) {
    int lane_min = SGM_INF;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        L[k] = C[k];
        lane_min = sgm_min(lane_min, L[k]);
    }
    m = sgm_wave_min(lane_min);
}

// ---- horizontal paths -----------------------------------------------------------------------------------------
// the base census word and the new window word of step i0 + lane (zeros past the row / outside the image)
GS2M_DEVICE void sgm_row_chunk(const unsigned long long* __restrict__ B, const unsigned long long* __restrict__ O, int W, int i0,
                               int lane, int x0, int s, int fresh_off, unsigned long long& base, unsigned long long& fresh) {
    const int i = i0 + lane;
    const int x = x0 + s * i;
    const int xf = x + fresh_off;
    base = i < W ? B[x] : 0ull;
    fresh = (i < W && xf >= 0 && xf < W) ? O[xf] : 0ull;
}

template <int K>
GS2M_KERNEL void __launch_bounds__(64)
k_sgm_horizontal(const unsigned long long* __restrict__ cen_base, const unsigned long long* __restrict__ cen_other, int W, int H,
                 int sgn, int P1, int P2, unsigned char* __restrict__ plane_fwd, unsigned char* __restrict__ plane_bwd) {
    constexpr int D = 64 * K;
    const int lane = gs2m_lane();
    const int row = (int)(blockIdx.x >> 1);
    const int dir = (int)(blockIdx.x & 1u);          // 0: left to right, 1: right to left
    if (row >= H) return;
    const unsigned long long* B = cen_base + (size_t)row * W;
    const unsigned long long* O = cen_other + (size_t)row * W;
    unsigned char* out = (dir ? plane_bwd : plane_fwd) + (size_t)row * W * D + lane * K;
    const int s = dir ? -1 : 1;
    const int x0 = dir ? W - 1 : 0;
    const int d0 = lane * K;
    // window: w[k] = O[x - sgn (d0 + k)].  One step moves x by s, i.e. the window by s sgn disparities: towards the
    // higher lanes (toward > 0: lane 0 takes the new word O[x]) or towards the lower ones (lane 63 takes O[x - sgn (D-1)]).
    const int toward = s * sgn;
    const int fresh_off = toward > 0 ? 0 : -sgn * (D - 1);
    unsigned long long w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int xo = x0 - sgn * (d0 + k);
        w[k] = (xo >= 0 && xo < W) ? O[xo] : 0ull;
    }
    unsigned long long cur_b, cur_f, nxt_b, nxt_f;
    sgm_row_chunk(B, O, W, 0, lane, x0, s, fresh_off, cur_b, cur_f);
    int L[K], C[K];
    int m = 0;
    for (int i0 = 0; i0 < W; i0 += 64) {
        sgm_row_chunk(B, O, W, i0 + 64, lane, x0, s, fresh_off, nxt_b, nxt_f);       // in flight during these 64 steps
        const int n = W - i0 < 64 ? W - i0 : 64;
        for (int j = 0; j < n; ++j) {
            const int i = i0 + j;
            const int x = x0 + s * i;
            const unsigned long long bc = gs2m_shfl(cur_b, j);
            if (i > 0) {
                const unsigned long long fr = gs2m_shfl(cur_f, j);
                if (toward > 0) {
                    unsigned long long in = gs2m_shfl_up(w[K - 1], 1);
                    if (lane == 0) in = fr;
#pragma unroll
                    for (int k = K - 1; k > 0; --k) w[k] = w[k - 1];
                    w[0] = in;
                } else {
                    unsigned long long in = gs2m_shfl(w[0], lane + 1);
                    if (lane == 63) in = fr;
#pragma unroll
                    for (int k = 0; k + 1 < K; ++k) w[k] = w[k + 1];
                    w[K - 1] = in;
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int xo = x - sgn * (d0 + k);
                C[k] = (xo >= 0 && xo < W) ? gs2m_popc64(bc ^ w[k]) : SGM_OOB_COST;
            }
            if (i == 0) sgm_path_first<K>(L, C, m);
            else sgm_path_step<K>(L, C, m, P1, P2, lane);
            SgmPack<unsigned char, K> o;
#pragma unroll
            for (int k = 0; k < K; ++k) o.v[k] = (unsigned char)L[k];
            *reinterpret_cast<SgmPack<unsigned char, K>*>(out + (size_t)x * D) = o;
        }
        cur_b = nxt_b;
        cur_f = nxt_f;
    }
}

// ---- vertical paths -------------------------------------------------------------------------------------------
// what a column kernel reads of one row: the base census word (wave-uniform) and the K window words of the lane
template <int K>
GS2M_DEVICE void sgm_col_census(const unsigned long long* __restrict__ cen_base, const unsigned long long* __restrict__ cen_other,
                                int W, int y, int x, const int (&xo)[K], unsigned long long& bc, unsigned long long (&w)[K]) {
    const size_t r = (size_t)y * W;
    bc = cen_base[r + x];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = cen_other[r + xo[k]];
}

template <int K>
GS2M_KERNEL void __launch_bounds__(64)
k_sgm_down(const unsigned long long* __restrict__ cen_base, const unsigned long long* __restrict__ cen_other, int W, int H, int sgn,
           int P1, int P2, const unsigned char* __restrict__ plane_fwd, const unsigned char* __restrict__ plane_bwd,
           unsigned short* __restrict__ sum) {
    constexpr int D = 64 * K;
    typedef SgmPack<unsigned char, K> P8;
    typedef SgmPack<unsigned short, K> P16;
    const int lane = gs2m_lane();
    const int x = gs2m_uniform((int)blockIdx.x);
    if (x >= W) return;
    const int d0 = lane * K;
    int xo[K];
    bool valid[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int t = x - sgn * (d0 + k);
        valid[k] = t >= 0 && t < W;
        xo[k] = valid[k] ? t : x;               // any word inside the row: its cost is replaced
    }
    const size_t lane_off = (size_t)x * D + d0;
    const size_t row_stride = (size_t)W * D;
    unsigned long long bc, w[K], nbc, nw[K];
    P8 hf, hb, nhf = {}, nhb = {};
    sgm_col_census<K>(cen_base, cen_other, W, 0, x, xo, bc, w);
    hf = *reinterpret_cast<const P8*>(plane_fwd + lane_off);
    hb = *reinterpret_cast<const P8*>(plane_bwd + lane_off);
    nbc = bc;
#pragma unroll
    for (int k = 0; k < K; ++k) nw[k] = w[k];
    int L[K], C[K];
    int m = 0;
    for (int y = 0; y < H; ++y) {
        if (y + 1 < H) {                       // the next row's loads, issued before this row's work
            sgm_col_census<K>(cen_base, cen_other, W, y + 1, x, xo, nbc, nw);
            nhf = *reinterpret_cast<const P8*>(plane_fwd + (size_t)(y + 1) * row_stride + lane_off);
            nhb = *reinterpret_cast<const P8*>(plane_bwd + (size_t)(y + 1) * row_stride + lane_off);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) C[k] = valid[k] ? gs2m_popc64(bc ^ w[k]) : SGM_OOB_COST;
        if (y == 0) sgm_path_first<K>(L, C, m);
        else sgm_path_step<K>(L, C, m, P1, P2, lane);
        P16 o;
#pragma unroll
        for (int k = 0; k < K; ++k) o.v[k] = (unsigned short)((int)hf.v[k] + (int)hb.v[k] + L[k]);
        *reinterpret_cast<P16*>(sum + (size_t)y * row_stride + lane_off) = o;
        bc = nbc;
        hf = nhf;
        hb = nhb;
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = nw[k];
    }
}

template <int K>
GS2M_KERNEL void __launch_bounds__(64)
k_sgm_up(const unsigned long long* __restrict__ cen_base, const unsigned long long* __restrict__ cen_other, int W, int H, int sgn,
         int P1, int P2, const unsigned short* __restrict__ sum, float* __restrict__ disp, unsigned short* __restrict__ tap) {
    constexpr int D = 64 * K;
    typedef SgmPack<unsigned short, K> P16;
    const int lane = gs2m_lane();
    const int x = gs2m_uniform((int)blockIdx.x);
    if (x >= W) return;
    const int d0 = lane * K;
    int xo[K];
    bool valid[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int t = x - sgn * (d0 + k);
        valid[k] = t >= 0 && t < W;
        xo[k] = valid[k] ? t : x;
    }
    const size_t lane_off = (size_t)x * D + d0;
    const size_t row_stride = (size_t)W * D;
    unsigned long long bc, w[K], nbc, nw[K];
    P16 sp3, nsp3 = {};
    sgm_col_census<K>(cen_base, cen_other, W, H - 1, x, xo, bc, w);
    sp3 = *reinterpret_cast<const P16*>(sum + (size_t)(H - 1) * row_stride + lane_off);
    nbc = bc;
#pragma unroll
    for (int k = 0; k < K; ++k) nw[k] = w[k];
    int L[K], C[K], S[K];
    int m = 0;
    for (int y = H - 1; y >= 0; --y) {
        if (y > 0) {
            sgm_col_census<K>(cen_base, cen_other, W, y - 1, x, xo, nbc, nw);
            nsp3 = *reinterpret_cast<const P16*>(sum + (size_t)(y - 1) * row_stride + lane_off);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) C[k] = valid[k] ? gs2m_popc64(bc ^ w[k]) : SGM_OOB_COST;
        if (y == H - 1) sgm_path_first<K>(L, C, m);
        else sgm_path_step<K>(L, C, m, P1, P2, lane);
        int key = 0x7fffffff;                  // (S << 10 | d): the minimum is the lowest d among the lowest S
#pragma unroll
        for (int k = 0; k < K; ++k) {
            S[k] = (int)sp3.v[k] + L[k];
            key = sgm_min(key, (S[k] << 10) | (d0 + k));
        }
        if (tap) {
            P16 o;
#pragma unroll
            for (int k = 0; k < K; ++k) o.v[k] = (unsigned short)S[k];
            *reinterpret_cast<P16*>(tap + (size_t)y * row_stride + lane_off) = o;
        }
        if (disp) {
            key = sgm_wave_min(key);
            const int best = key & 1023;
            const int dm = best > 0 ? best - 1 : 0, dp = best < D - 1 ? best + 1 : D - 1;
            int pick_m = 0, pick_p = 0;        // S[dm % K], S[dp % K] of every lane; the owning lane's is the one read
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k == dm % K) pick_m = S[k];
                if (k == dp % K) pick_p = S[k];
            }
            const float sm = (float)gs2m_shfl(pick_m, dm / K);
            const float sp = (float)gs2m_shfl(pick_p, dp / K);
            const float s0 = (float)(key >> 10);
            const float den = sm + sp - 2.0f * s0;
            float d = (float)best;
            if (best > 0 && best < D - 1 && den > 0.0f) d = d + (sm - sp) / (2.0f * den);
            if (lane == 0) disp[(size_t)y * W + x] = d;
        }
        bc = nbc;
        sp3 = nsp3;
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = nw[k];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
struct SgmScratch {
    unsigned char* grey;                  // [2][H][W]
    unsigned long long* census;           // [2][H][W]
    unsigned char *plane_fwd, *plane_bwd; // [H][W][D] u8 each
    unsigned short* sum;                  // [H][W][D] u16
    int64_t bytes;
};

static inline SgmScratch sgm_scratch_layout(void* base, int W, int H, int D) {
    const int64_t n = (int64_t)W * H;
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    SgmScratch s;
    int64_t o = 0;
    unsigned char* b = (unsigned char*)base;
    s.grey = b + o;
    o += up(2 * n);
    s.census = (unsigned long long*)(b + o);
    o += up(2 * n * 8);
    s.plane_fwd = b + o;
    o += up(n * D);
    s.plane_bwd = b + o;
    o += up(n * D);
    s.sum = (unsigned short*)(b + o);
    o += up(n * D * 2);
    s.bytes = o;
    return s;
}

template <int K>
static void sgm_launch_pass(hipStream_t stream, const unsigned long long* cen_base, const unsigned long long* cen_other, int W, int H,
                            int sgn, int P1, int P2, const SgmScratch& s, float* disp, unsigned short* tap) {
    GS2M_LAUNCH(k_sgm_horizontal<K>, dim3(2u * (unsigned)H), dim3(64), 0, stream, cen_base, cen_other, W, H, sgn, P1, P2,
                s.plane_fwd, s.plane_bwd);
    GS2M_LAUNCH(k_sgm_down<K>, dim3((unsigned)W), dim3(64), 0, stream, cen_base, cen_other, W, H, sgn, P1, P2,
                (const unsigned char*)s.plane_fwd, (const unsigned char*)s.plane_bwd, s.sum);
    GS2M_LAUNCH(k_sgm_up<K>, dim3((unsigned)W), dim3(64), 0, stream, cen_base, cen_other, W, H, sgn, P1, P2,
                (const unsigned short*)s.sum, disp, tap);
}

static void sgm_launch(hipStream_t stream, const unsigned char* left, const unsigned char* right, int W, int H, int D, int P1, int P2,
                       float* disp_lr, float* disp_rl, const SgmScratch& s, unsigned short* tap) {
    const int n = W * H;
    GS2M_LAUNCH(k_sgm_grey, dim3((n + 255) / 256, 2), dim3(256), 0, stream, left, right, n, s.grey);
    GS2M_LAUNCH(k_sgm_census, dim3((W + 255) / 256, H, 2), dim3(256), 0, stream, (const unsigned char*)s.grey, W, H, s.census);
    const unsigned long long* cl = s.census;
    const unsigned long long* cr = s.census + (size_t)n;
    for (int pass = 0; pass < 2; ++pass) {
        float* disp = pass ? disp_rl : disp_lr;
        unsigned short* t = pass ? nullptr : tap;
        if (!disp && !t) continue;
        const unsigned long long* cb = pass ? cr : cl;
        const unsigned long long* co = pass ? cl : cr;
        const int sgn = pass ? -1 : 1;
        switch (D / 64) {
#define SGM_CASE(K) case K: sgm_launch_pass<K>(stream, cb, co, W, H, sgn, P1, P2, s, disp, t); break;
            SGM_CASE(1) SGM_CASE(2) SGM_CASE(3) SGM_CASE(4) SGM_CASE(5) SGM_CASE(6) SGM_CASE(7) SGM_CASE(8)
            SGM_CASE(9) SGM_CASE(10) SGM_CASE(11) SGM_CASE(12) SGM_CASE(13) SGM_CASE(14) SGM_CASE(15) SGM_CASE(16)
#undef SGM_CASE
        }
    }
}
