// mask_disk_kernels.h -- binary dilation of n masks with a disk of radius r on the packed bitmaps of mask_kernels.h: the
// `binary_dilation(mask, disk(24))` of the DTU evaluation's cull_scan (evaluation/DTU/eval_code/evaluate_single_scene.py:80),
// which is scipy.ndimage.binary_dilation with the (2r + 1)^2 footprint dy^2 + dx^2 <= r^2 and a 0 border:
//   out(y, x) = OR over dy^2 + dx^2 <= r^2 of in(y + dy, x + dx),  in = 0 outside the image.
//
// A disk is a stack of horizontal runs: row dy has the half-width w(dy) = floor(sqrt(r^2 - dy^2)), which falls as |dy| grows,
// and a row dilation by a + b is the row dilation by a of the row dilation by b (on the unbounded line: a bit that walks out
// of the image and back has moved no farther than one that stayed).  So the disk is applied Horner-wise from the centre row
// outwards,
//   A = in[y];   for d = 0 .. r - 1:  A = rowdil(A, w(d) - w(d + 1)) | in[y - d - 1] | in[y + d + 1]      (w(r) = 0),
// which gives row y +- d the total half-width w(d) in r one-pixel steps altogether (the sum of the differences is w(0) = r)
// instead of 2r + 1 separate row dilations.  One thread per output word keeps A as three words, its own and both neighbours:
// no bit travels farther than r <= 64 pixels, so what the neighbours lack from THEIR far neighbours can never reach the own
// word.  Rows outside the image are the 0 border and are not read.  The steps w(d) - w(d + 1) travel in the kernel arguments.
#pragma once
#include "mask_kernels.h"

#define GS2M_DISK_MAX_RADIUS 64

struct DiskSteps {
    unsigned char k[GS2M_DISK_MAX_RADIUS];        // k[d] = w(d) - w(d + 1), d < r
};

// words w - 1, w, w + 1 of a bitmap row; 0 outside the row
struct MaskWords3 {
    unsigned long long lo, mid, hi;
};
GS2M_DEVICE MaskWords3 mask_words3(const unsigned long long* __restrict__ row, int w, int nw) {
    MaskWords3 a;
    a.lo = w > 0 ? row[w - 1] : 0ull;
    a.mid = row[w];
    a.hi = w + 1 < nw ? row[w + 1] : 0ull;
    return a;
}

// src: [nf][H][nw] packed masks (bits at x >= W are 0).  dst: [nf][H][nw], the dilated bitmaps, bits at x >= W cleared.
GS2M_KERNEL void __launch_bounds__(256)
k_mask_dilate_disk(DiskSteps S, int r, int W, int H, int nw, const unsigned long long* __restrict__ src,
                   unsigned long long* __restrict__ dst) {
    const int f = (int)blockIdx.y;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)H * nw) return;
    const int y = (int)(g / nw), w = (int)(g - (long long)y * nw);
    const unsigned long long* frame = src + (size_t)f * H * nw;
    MaskWords3 A = mask_words3(frame + (size_t)y * nw, w, nw);
    for (int d = 0; d < r; ++d) {
        for (int j = S.k[d]; j > 0; --j) {                           // one pixel to either side
            MaskWords3 n;
            n.lo = A.lo | (A.lo << 1) | (A.lo >> 1) | (A.mid << 63);
            n.mid = A.mid | (A.mid << 1) | (A.lo >> 63) | (A.mid >> 1) | (A.hi << 63);
            n.hi = A.hi | (A.hi << 1) | (A.mid >> 63) | (A.hi >> 1);
            A = n;
        }
        const int up = y - d - 1, down = y + d + 1;
        if (up >= 0) {
            const MaskWords3 t = mask_words3(frame + (size_t)up * nw, w, nw);
            A.lo |= t.lo;
            A.mid |= t.mid;
            A.hi |= t.hi;
        }
        if (down < H) {
            const MaskWords3 t = mask_words3(frame + (size_t)down * nw, w, nw);
            A.lo |= t.lo;
            A.mid |= t.mid;
            A.hi |= t.hi;
        }
    }
    unsigned long long v = A.mid;
    if (w == nw - 1 && (W & 63)) v &= (1ull << (W & 63)) - 1ull;
    dst[(size_t)f * H * nw + g] = v;
}

// bytes: [nf][H][W] 0 / 1 from bits [nf][H][nw].  Thread per pixel (the byte form is for inspection and tests).
GS2M_KERNEL void __launch_bounds__(256)
k_mask_bits_to_bytes(int W, int H, int nw, const unsigned long long* __restrict__ bits, unsigned char* __restrict__ bytes) {
    const int f = (int)blockIdx.y;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const unsigned long long word = bits[((size_t)f * H + y) * nw + (x >> 6)];
    bytes[(size_t)f * H * W + p] = (unsigned char)((word >> (x & 63)) & 1ull);
}

// k[d] = w(d) - w(d + 1) with w(d) = floor(sqrt(r^2 - d^2)) in integers
static inline DiskSteps gs2m_disk_steps(int r) {
    DiskSteps S;
    int w[GS2M_DISK_MAX_RADIUS + 1];
    for (int d = 0; d <= r; ++d) {
        int q = 0;
        while ((q + 1) * (q + 1) + d * d <= r * r) ++q;
        w[d] = q;
    }
    for (int d = 0; d < GS2M_DISK_MAX_RADIUS; ++d) S.k[d] = d < r ? (unsigned char)(w[d] - w[d + 1]) : 0;
    return S;
}

// one chunk of nf <= GS2M_MASK_BATCH masks: pack into in_bits [nf][H][nw], dilate into out_bits [nf][H][nw], and write the
// bytes [nf][H][W] when asked
static inline void gs2m_launch_mask_dilate_disk(hipStream_t st, const unsigned char* const* masks, int nf, int W, int H, int r,
                                                unsigned long long* in_bits, unsigned long long* out_bits, unsigned char* out_bytes) {
    const int nw = (W + 63) / 64;
    const long long words = (long long)H * nw;
    MaskBatch B;
    bool vec = (W & 15) == 0;
    for (int i = 0; i < GS2M_MASK_BATCH; ++i) {
        B.obj[i] = i < nf ? masks[i] : nullptr;
        B.occ[i] = nullptr;
        B.out[i] = nullptr;
        vec = vec && ((uintptr_t)B.obj[i] & 15u) == 0;
    }
    const dim3 gw((unsigned)((words + 3) / 4), (unsigned)nf), gt((unsigned)((words + 255) / 256), (unsigned)nf);
    if (vec) GS2M_LAUNCH(k_mask_pack16, gt, dim3(256), 0, st, B, W, H, nw, 0, in_bits);
    else GS2M_LAUNCH(k_mask_pack, gw, dim3(256), 0, st, B, W, H, nw, 0, in_bits);
    GS2M_LAUNCH(k_mask_dilate_disk, gt, dim3(256), 0, st, gs2m_disk_steps(r), r, W, H, nw, (const unsigned long long*)in_bits, out_bits);
    if (out_bytes)
        GS2M_LAUNCH(k_mask_bits_to_bytes, dim3((unsigned)(((long long)H * W + 255) / 256), (unsigned)nf), dim3(256), 0, st, W, H, nw,
                    (const unsigned long long*)out_bits, out_bytes);
}
