// loss_kernels.h -- gs2m_photo_loss_forward / _backward: the photometric loss of 3DGS training,
//   loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean(ssim_map(x, y)))
// (GS/utils/loss_utils.py, train.py:89-90), as two tiled kernels and one small reduction instead of torch's five grouped
// 11 x 11 convolutions, their element-wise chain and the same again in reverse.  Window: 11 taps, Gaussian, sigma 1.5,
// normalised; zero padding; per plane; C1 = 0.01^2, C2 = 0.03^2.
//
// Tile.  One workgroup of 256 threads owns a tile of LOSS_TW x LOSS_TH = 32 x 16 pixels of one plane.  32 wide: a wave's 64
// lanes read two full rows of 32 consecutive floats, so the vertical pass over the row-filtered planes (row stride 32) touches
// all 64 LDS banks once, and global rows are read and written in 128-byte pieces.  16 high: the horizontal pass runs on
// 16 + 10 rows, 1.6 x the tile, where 8 rows would make it 2.25 x.  LDS per workgroup: forward 2 * 26 * 42 (x, y with halo)
// + 5 * 26 * 32 (row-filtered x, y, xx, yy, xy) + 2 * 256 (reduction) floats = 27 424 bytes, backward 3 * 26 * 42 + 3 * 26 * 32
// floats = 23 088 bytes: five workgroups per CU in the forward and seven in the backward, 20 and 28 waves (the compiler's
// occupancy of 5 and 7 waves per SIMD).
//
// Arithmetic (include/gs2mesh_amd.h states it; tests/loss_statement.py restates it in numpy).  This header is compiled into
// train_kernels.hip, built with -ffp-contract=off: every operation below is one f32 operation rounded on its own, divisions
// are IEEE divisions, and parentheses are the order.  w[0..10] come from the host (double, normalised, cast to f32).
//   filter    F(q)(r, c) = V(H(q)):  H(q)(r, c) = sum_k w[k] * q(r, c + k - 5),  V(h)(r, c) = sum_k w[k] * h(r + k - 5, c),
//             each sum  acc = 0; for k = 0 .. 10: acc = acc + w[k] * term_k;  q and H(q) are 0 outside the image
//   moments   mu1 = F(x), mu2 = F(y), exx = F(x * x), eyy = F(y * y), exy = F(x * y)
//             m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2, s1 = exx - m11, s2 = eyy - m22, s12 = exy - m12
//   map       A = (m11 + m22) + C1, B = (s1 + s2) + C2, C = 2 * m12 + C1, D = 2 * s12 + C2, AB = A * B, m = (C * D) / AB
//   partials  p0 = dm/dmu1 = 2 * ((((mu2 * D) / AB - (mu2 * C) / AB) - (mu1 * m) / A) + (mu1 * m) / B)
//             p1 = dm/dsigma1^2 = -(m / B),   p2 = dm/dsigma12 = (2 * C) / AB
//   backward  gl = grad_loss[0], g = gl * (-kb), l = gl * ka  with  ka = f32((1 - lambda) / N), kb = f32(lambda / N) from the host
//             dx = ((F(g * p0) + (2 * x) * F(g * p1)) + y * F(g * p2)) + l * sign(x - y),  sign = (d > 0) - (d < 0)
//   scalars   S1 = sum |x - y|, Sm = sum m;  out = { (ka * S1 + f32(lambda)) - kb * Sm,  S1 * f32(1 / N),  Sm * f32(1 / N) }
//
// Sums.  No float atomics.  A thread adds its two pixels to zero in row order (2 additions), the 256 threads of a tile are
// added by a tree in LDS (8), the tile's pair goes to scratch; the single workgroup of k_loss_final gives each of its 1024
// threads the tiles t, t + 1024, ... in that order (ceil(tiles / 1024) additions) and adds the threads by a tree (10).  The
// longest addition chain is therefore LOSS_CHAIN(tiles) = 2 + 8 + ceil(tiles / 1024) + 10, and the order is fixed: the same
// bits on every run.  The three results take at most 4 more roundings each (the products with the host's factors and the
// two additions of out[0]); the tests bound them by LOSS_CHAIN alone, without an allowance for these.
#pragma once

#define LOSS_TW 32
#define LOSS_TH 16
#define LOSS_R 5
#define LOSS_TAPS (2 * LOSS_R + 1)
#define LOSS_RW (LOSS_TW + 2 * LOSS_R)
#define LOSS_RH (LOSS_TH + 2 * LOSS_R)
#define LOSS_THREADS 256
#define LOSS_FINAL_THREADS 1024
#define LOSS_MAX_TILES (1 << 23)          // 2^32 pixels of whole tiles; keeps the 1-D grid far from the launch limits

struct LossWindow {
    float w[LOSS_TAPS];
};

struct LossTiling {
    int ntx, nty;
    int64_t tiles;                        // planes * nty * ntx
};

static inline LossTiling loss_tiling(int planes, int H, int W) {
    LossTiling g;
    const int64_t ntx = ((int64_t)W + LOSS_TW - 1) / LOSS_TW, nty = ((int64_t)H + LOSS_TH - 1) / LOSS_TH;
    g.ntx = (int)ntx;                     // both fit: at most 2^31 / 16
    g.nty = (int)nty;
    // planes * nty * ntx without leaving int64: anything over the limit is reported as the limit + 1
    g.tiles = ntx * nty > LOSS_MAX_TILES ? (int64_t)LOSS_MAX_TILES + 1 : (int64_t)planes * (ntx * nty);
    if (g.tiles > LOSS_MAX_TILES) g.tiles = (int64_t)LOSS_MAX_TILES + 1;
    return g;
}

// normalised Gaussian, sigma 1.5, in double as training._window writes it; cast to f32 last
static inline LossWindow loss_window() {
    double g[LOSS_TAPS], sum = 0.0;
    for (int i = 0; i < LOSS_TAPS; ++i) {
        g[i] = exp(-(double)((i - LOSS_R) * (i - LOSS_R)) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    LossWindow win;
    for (int i = 0; i < LOSS_TAPS; ++i) win.w[i] = (float)(g[i] / sum);
    return win;
}

// load the LOSS_RH x LOSS_RW region around the tile at (r0, c0) into LDS, `scale` * value, zero outside the image
GS2M_DEVICE void loss_load_region(float* dst, const float* __restrict__ src, int H, int W, int r0, int c0, float scale,
                                  bool scaled) {
    for (int i = (int)threadIdx.x; i < LOSS_RH * LOSS_RW; i += LOSS_THREADS) {
        const int r = r0 + i / LOSS_RW - LOSS_R, c = c0 + i % LOSS_RW - LOSS_R;
        float v = 0.0f;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            v = src[(size_t)r * W + c];
            if (scaled) v = scale * v;
        }
        dst[i] = v;
    }
}

GS2M_DEVICE void loss_tile_of_block(int ntx, int nty, int& plane, int& r0, int& c0) {
    const int tile = (int)blockIdx.x;
    c0 = (tile % ntx) * LOSS_TW;
    r0 = ((tile / ntx) % nty) * LOSS_TH;
    plane = tile / (ntx * nty);
}

GS2M_KERNEL void __launch_bounds__(LOSS_THREADS)
k_loss_forward(int H, int W, int ntx, int nty, int64_t total, const float* __restrict__ x, const float* __restrict__ y,
               LossWindow win, float* __restrict__ tile_sums, float* __restrict__ partials, float* __restrict__ tap) {
    __shared__ float sx[LOSS_RH * LOSS_RW], sy[LOSS_RH * LOSS_RW];
    __shared__ float hq[5][LOSS_RH * LOSS_TW];
    __shared__ float red[2][LOSS_THREADS];
    const int t = (int)threadIdx.x;
    int plane, r0, c0;
    loss_tile_of_block(ntx, nty, plane, r0, c0);
    const size_t base = (size_t)plane * H * W;
    loss_load_region(sx, x + base, H, W, r0, c0, 0.0f, false);
    loss_load_region(sy, y + base, H, W, r0, c0, 0.0f, false);
    __syncthreads();
    for (int i = t; i < LOSS_RH * LOSS_TW; i += LOSS_THREADS) {
        const float* px = sx + (i / LOSS_TW) * LOSS_RW + i % LOSS_TW;
        const float* py = sy + (i / LOSS_TW) * LOSS_RW + i % LOSS_TW;
        float ax = 0.0f, ay = 0.0f, axx = 0.0f, ayy = 0.0f, axy = 0.0f;
#pragma unroll
        for (int k = 0; k < LOSS_TAPS; ++k) {
            const float w = win.w[k], a = px[k], b = py[k];
            ax = ax + w * a;
            ay = ay + w * b;
            axx = axx + w * (a * a);
            ayy = ayy + w * (b * b);
            axy = axy + w * (a * b);
        }
        hq[0][i] = ax, hq[1][i] = ay, hq[2][i] = axx, hq[3][i] = ayy, hq[4][i] = axy;
    }
    __syncthreads();
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float l1 = 0.0f, sm = 0.0f;
    for (int i = t; i < LOSS_TH * LOSS_TW; i += LOSS_THREADS) {
        const int rr = i / LOSS_TW, cc = i % LOSS_TW, r = r0 + rr, c = c0 + cc;
        if (r >= H || c >= W) continue;
        float mu1 = 0.0f, mu2 = 0.0f, exx = 0.0f, eyy = 0.0f, exy = 0.0f;
#pragma unroll
        for (int k = 0; k < LOSS_TAPS; ++k) {
            const float w = win.w[k];
            const int j = (rr + k) * LOSS_TW + cc;
            mu1 = mu1 + w * hq[0][j];
            mu2 = mu2 + w * hq[1][j];
            exx = exx + w * hq[2][j];
            eyy = eyy + w * hq[3][j];
            exy = exy + w * hq[4][j];
        }
        const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
        const float s1 = exx - m11, s2 = eyy - m22, s12 = exy - m12;
        const float A = (m11 + m22) + C1, B = (s1 + s2) + C2, C = 2.0f * m12 + C1, D = 2.0f * s12 + C2;
        const float AB = A * B;
        const float m = (C * D) / AB;
        const float a = sx[(rr + LOSS_R) * LOSS_RW + cc + LOSS_R], b = sy[(rr + LOSS_R) * LOSS_RW + cc + LOSS_R];
        l1 = l1 + fabsf(a - b);
        sm = sm + m;
        const size_t p = base + (size_t)r * W + c;
        if (tap) tap[p] = m;
        if (partials) {
            const float mu1m = mu1 * m;
            partials[p] = 2.0f * ((((mu2 * D) / AB - (mu2 * C) / AB) - mu1m / A) + mu1m / B);
            partials[(size_t)total + p] = -(m / B);
            partials[2 * (size_t)total + p] = (2.0f * C) / AB;
        }
    }
    red[0][t] = l1, red[1][t] = sm;
    __syncthreads();
    for (int s = LOSS_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            red[0][t] = red[0][t] + red[0][t + s];
            red[1][t] = red[1][t] + red[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        tile_sums[2 * (size_t)blockIdx.x] = red[0][0];
        tile_sums[2 * (size_t)blockIdx.x + 1] = red[1][0];
    }
}

GS2M_KERNEL void __launch_bounds__(LOSS_FINAL_THREADS)
k_loss_final(int tiles, const float* __restrict__ tile_sums, float ka, float kb, float lambda, float inv_n,
             float* __restrict__ out) {
    __shared__ float red[2][LOSS_FINAL_THREADS];
    const int t = (int)threadIdx.x;
    float s1 = 0.0f, sm = 0.0f;
    for (int i = t; i < tiles; i += LOSS_FINAL_THREADS) {
        s1 = s1 + tile_sums[2 * (size_t)i];
        sm = sm + tile_sums[2 * (size_t)i + 1];
    }
    red[0][t] = s1, red[1][t] = sm;
    __syncthreads();
    for (int s = LOSS_FINAL_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            red[0][t] = red[0][t] + red[0][t + s];
            red[1][t] = red[1][t] + red[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        s1 = red[0][0], sm = red[1][0];
        out[0] = (ka * s1 + lambda) - kb * sm;
        out[1] = s1 * inv_n;
        out[2] = sm * inv_n;
    }
}

GS2M_KERNEL void __launch_bounds__(LOSS_THREADS)
k_loss_backward(int H, int W, int ntx, int nty, int64_t total, const float* __restrict__ x, const float* __restrict__ y,
                const float* __restrict__ partials, LossWindow win, float ka, float kb, const float* __restrict__ grad_loss,
                float* __restrict__ grad_x) {
    __shared__ float sp[3][LOSS_RH * LOSS_RW];
    __shared__ float hq[3][LOSS_RH * LOSS_TW];
    const int t = (int)threadIdx.x;
    int plane, r0, c0;
    loss_tile_of_block(ntx, nty, plane, r0, c0);
    const size_t base = (size_t)plane * H * W;
    const float gl = grad_loss[0];
    const float g = gl * (-kb), l = gl * ka;
    for (int q = 0; q < 3; ++q) loss_load_region(sp[q], partials + (size_t)q * (size_t)total + base, H, W, r0, c0, g, true);
    __syncthreads();
    for (int i = t; i < LOSS_RH * LOSS_TW; i += LOSS_THREADS) {
        const int o = (i / LOSS_TW) * LOSS_RW + i % LOSS_TW;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
        for (int k = 0; k < LOSS_TAPS; ++k) {
            const float w = win.w[k];
            a0 = a0 + w * sp[0][o + k];
            a1 = a1 + w * sp[1][o + k];
            a2 = a2 + w * sp[2][o + k];
        }
        hq[0][i] = a0, hq[1][i] = a1, hq[2][i] = a2;
    }
    __syncthreads();
    for (int i = t; i < LOSS_TH * LOSS_TW; i += LOSS_THREADS) {
        const int rr = i / LOSS_TW, cc = i % LOSS_TW, r = r0 + rr, c = c0 + cc;
        if (r >= H || c >= W) continue;
        float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
#pragma unroll
        for (int k = 0; k < LOSS_TAPS; ++k) {
            const float w = win.w[k];
            const int j = (rr + k) * LOSS_TW + cc;
            f0 = f0 + w * hq[0][j];
            f1 = f1 + w * hq[1][j];
            f2 = f2 + w * hq[2][j];
        }
        const size_t p = base + (size_t)r * W + c;
        const float a = x[p], b = y[p], d = a - b;
        const float sign = (float)((d > 0.0f) - (d < 0.0f));
        grad_x[p] = ((f0 + (2.0f * a) * f1) + b * f2) + l * sign;
    }
}

static void loss_launch_forward(hipStream_t stream, int planes, int H, int W, const float* x, const float* y, float lambda,
                                float* tile_sums, float* out, float* partials, float* tap) {
    const LossTiling g = loss_tiling(planes, H, W);
    const int64_t total = (int64_t)planes * H * W;
    const double n = (double)total;
    const LossWindow win = loss_window();
    const float ka = (float)((1.0 - (double)lambda) / n), kb = (float)((double)lambda / n), inv_n = (float)(1.0 / n);
    const int ntx = g.ntx, nty = g.nty, tiles = (int)g.tiles;
    GS2M_LAUNCH(k_loss_forward, dim3((unsigned)tiles), dim3(LOSS_THREADS), 0, stream, H, W, ntx, nty, total, x, y, win, tile_sums,
                partials, tap);
    GS2M_LAUNCH(k_loss_final, dim3(1), dim3(LOSS_FINAL_THREADS), 0, stream, tiles, (const float*)tile_sums, ka, kb, lambda, inv_n,
                out);
}

static void loss_launch_backward(hipStream_t stream, int planes, int H, int W, const float* x, const float* y,
                                 const float* partials, float lambda, const float* grad_loss, float* grad_x) {
    const LossTiling g = loss_tiling(planes, H, W);
    const int64_t total = (int64_t)planes * H * W;
    const double n = (double)total;
    const LossWindow win = loss_window();
    const float ka = (float)((1.0 - (double)lambda) / n), kb = (float)((double)lambda / n);
    const int ntx = g.ntx, nty = g.nty, tiles = (int)g.tiles;
    GS2M_LAUNCH(k_loss_backward, dim3((unsigned)tiles), dim3(LOSS_THREADS), 0, stream, H, W, ntx, nty, total, x, y, partials, win,
                ka, kb, grad_loss, grad_x);
}
