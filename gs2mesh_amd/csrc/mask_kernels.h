// mask_kernels.h -- object-mask preprocessing of TSDF.run on the device (gs2mesh_utils/tsdf_utils.py:69-83), n frames per call:
//   m   = object_mask != 0, inverted on request
//   m   = erode_k2(close_k1(m))        cv2.MORPH_CLOSE (dilate, then erode) and cv2.erode with k x k boxes of ones
//   out = m & (occlusion_mask != 0)    0 / 1 bytes
// bit-identical to the host statement gs2mesh_amd/tsdf_utils.py (preprocess_object_mask / _morph): the box window of every
// pixel is [x - k/2, x + k - 1 - k/2] in both axes, and each of the three operations pads with its own border value (erosion
// sees 1 outside the image, dilation 0).
//
// Every operation is written as a dilation with a 0 border: erode(x) = ~dilate(~x) when erode pads with 1, so
//   d1 = D_k1(m),  d2 = D_k1(~d1),  d3 = D_k2(d2),  result = ~d3.
// The masks are packed into 64-pixel words (one wave64 ballot per word; bits at x >= W are 0), and each 2-D box is a row pass
// (thread per word: shifts that reach into the neighbouring words, see k_mask_dilate_rows) followed by a column pass (thread
// per word: OR of the rows of the clipped window).  Reading 0 outside the image IS the 0 border.  Two scratch bitmaps per frame
// alternate between the passes; only the packing (bytes in) and the output (bytes out) touch every pixel.
#pragma once
#include "platform.h"

#define GS2M_MASK_BATCH 32   // frames per launch (the descriptor travels by value in the kernel arguments)

struct MaskBatch {
    const unsigned char* obj[GS2M_MASK_BATCH];   // NULL: no object mask for this frame
    const unsigned char* occ[GS2M_MASK_BATCH];   // NULL: no occlusion mask
    unsigned char* out[GS2M_MASK_BATCH];         // NULL: neither mask (the frame is not touched)
};

// row y of frame f in a scratch bitmap: [frames][H][nw] words
GS2M_DEVICE unsigned long long* mask_row(unsigned long long* bits, int f, int H, int nw, int y) {
    return bits + ((size_t)f * H + y) * nw;
}

// pack: bit x of word (y, w) = (obj[y][x] != 0) ^ invert.  One wave per word (flattened over rows), lane = bit.
GS2M_KERNEL void __launch_bounds__(256)
k_mask_pack(MaskBatch B, int W, int H, int nw, int invert, unsigned long long* __restrict__ bits) {
    const int f = (int)blockIdx.y;
    const unsigned char* obj = B.obj[f];
    if (!obj) return;                                                // block-uniform
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (long long)H * nw) return;                              // wave-uniform
    const int y = (int)(g / nw), w = (int)(g - (long long)y * nw);
    const int x = 64 * w + gs2m_lane();
    const bool on = x < W && ((obj[(size_t)y * W + x] != 0) != (invert != 0));
    const unsigned long long word = gs2m_ballot(on ? 1 : 0);
    if (gs2m_lane() == 0) mask_row(bits, f, H, nw, y)[w] = word;
}

// any set bit of (flip ? ~row : row) in [lo, hi] (0 <= lo <= hi < W: the bits at x >= W are never looked at)
GS2M_DEVICE bool mask_range_any(const unsigned long long* __restrict__ row, int lo, int hi, bool flip) {
    const int wl = lo >> 6, wh = hi >> 6;
    for (int q = wl; q <= wh; ++q) {
        unsigned long long v = row[q];
        if (flip) v = ~v;
        if (q == wl) v &= ~0ull << (lo & 63);
        if (q == wh) v &= ~0ull >> (63 - (hi & 63));
        if (v) return true;
    }
    return false;
}

// word q of a row as a dilation reads it: 0 outside the row (the border), complemented on request, bits at x >= W cleared
GS2M_DEVICE unsigned long long mask_word(const unsigned long long* __restrict__ row, long long q, int nw, int W, bool flip) {
    if (q < 0 || q >= nw) return 0ull;
    unsigned long long v = row[q];
    if (flip) v = ~v;
    if (q == nw - 1 && (W & 63)) v &= (1ull << (W & 63)) - 1ull;
    return v;
}
// the 64 bits of the row starting at bit p (any p; bit i of the result = pixel p + i)
GS2M_DEVICE unsigned long long mask_bits_at(const unsigned long long* __restrict__ row, long long p, int nw, int W, bool flip) {
    const long long q = p >> 6;                     // floor(p / 64), also for p < 0
    const int s = (int)(p & 63);
    const unsigned long long lo = mask_word(row, q, nw, W, flip);
    return s ? (lo >> s) | (mask_word(row, q + 1, nw, W, flip) << (64 - s)) : lo;
}

// row pass of a 0-border dilation: dst(y, x) = any src(y, x') for x' in [x - a, x - a + k - 1].  flip: the source is read
// complemented (~d1 of the closing's erosion).  One thread per output word: bit j of word w looks at the bits [P + j, P + j + k - 1]
// of the row, P = 64 w - a.
//   k <= 64: the 128 bits from P in two words, OR-ed with themselves shifted by 1, 2, 4, ... (doubling: bit i then covers a
//            window of L = the largest power of two <= k), and once more shifted by k - L (OR is idempotent: the two windows of
//            L overlap to exactly k).
//   k > 64:  bits [P + 63, P + k - 1] are in every window of the word: if one is set the word is all ones; else bit j = any of
//            [P + j, P + 62] (suffix OR of the word at P) or of [P + k, P + k + j - 1] (exclusive prefix OR of the word at P + k).
GS2M_KERNEL void __launch_bounds__(256)
k_mask_dilate_rows(unsigned frames, int W, int H, int nw, int a, int k, int flip, const unsigned long long* __restrict__ src,
                   unsigned long long* __restrict__ dst) {
    const int f = (int)blockIdx.y;
    if (!((frames >> f) & 1u)) return;                               // block-uniform
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)H * nw) return;
    const int y = (int)(g / nw), w = (int)(g - (long long)y * nw);
    const unsigned long long* row = src + ((size_t)f * H + y) * nw;
    const bool fl = flip != 0;
    const long long P = 64ll * w - a;
    unsigned long long r;
    if (k <= 64) {
        unsigned long long lo = mask_bits_at(row, P, nw, W, fl), hi = mask_bits_at(row, P + 64, nw, W, fl);
        int L = 1;
        for (; 2 * L <= k; L *= 2) {                                 // shifts of 1 .. 32
            lo |= (lo >> L) | (hi << (64 - L));
            hi |= hi >> L;
        }
        const int s = k - L;                                         // 0 <= s < L
        r = s ? lo | (lo >> s) | (hi << (64 - s)) : lo;
    } else {
        const long long m0 = P + 63 < 0 ? 0 : P + 63, m1 = P + k - 1 > W - 1 ? W - 1 : P + k - 1;
        if (m0 <= m1 && mask_range_any(row, (int)m0, (int)m1, fl)) {
            r = ~0ull;
        } else {
            unsigned long long sfx = mask_bits_at(row, P, nw, W, fl), pfx = mask_bits_at(row, P + k, nw, W, fl);
            for (int d = 1; d < 64; d *= 2) {
                sfx |= sfx >> d;
                pfx |= pfx << d;
            }
            r = sfx | (pfx << 1);
        }
    }
    if (w == nw - 1 && (W & 63)) r &= (1ull << (W & 63)) - 1ull;
    mask_row(dst, f, H, nw, y)[w] = r;
}

// column pass: dst(y, w) = OR of src(y', w) for y' in [y - a, y + b] clipped to the image.  Thread per word.
GS2M_KERNEL void __launch_bounds__(256)
k_mask_dilate_cols(unsigned frames, int H, int nw, int a, int b, const unsigned long long* __restrict__ src,
                   unsigned long long* __restrict__ dst) {
    const int f = (int)blockIdx.y;
    if (!((frames >> f) & 1u)) return;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)H * nw) return;
    const int y = (int)(g / nw), w = (int)(g - (long long)y * nw);
    const int lo = y - a < 0 ? 0 : y - a;
    const int hi = y > H - 1 - b ? H - 1 : y + b;
    const unsigned long long* s = src + (size_t)f * H * nw + w;
    unsigned long long v = 0ull;
    for (int r = lo; r <= hi; ++r) v |= s[(size_t)r * nw];
    dst[(size_t)f * H * nw + g] = v;
}

// output: out = object part & (occ != 0), 0 / 1.  The object part is ~d3 (bits != NULL), the raw mask (no morphology) or 1 (no
// object mask).  Thread per pixel.
GS2M_KERNEL void __launch_bounds__(256)
k_mask_output(MaskBatch B, int W, int H, int nw, int invert, const unsigned long long* __restrict__ bits) {
    const int f = (int)blockIdx.z, y = (int)blockIdx.y;
    const int x = (int)(blockIdx.x * 256u + threadIdx.x);
    unsigned char* out = B.out[f];
    if (!out || x >= W) return;
    const size_t p = (size_t)y * W + x;
    const unsigned char* obj = B.obj[f];
    const unsigned char* occ = B.occ[f];
    bool m = true;
    if (obj) {
        if (bits) m = !((bits[((size_t)f * H + y) * nw + (x >> 6)] >> (x & 63)) & 1ull);
        else m = (obj[p] != 0) != (invert != 0);
    }
    if (occ) m = m && occ[p] != 0;
    out[p] = m ? 1 : 0;
}

// ---- the byte ends, 16 pixels per load / store (width a multiple of 16, every mask 16-byte aligned: the usual case) ----------
// bit i = byte i of v is non-zero
GS2M_DEVICE unsigned mask_nz4(unsigned v) {
    return (unsigned)((v & 0xffu) != 0u) | ((unsigned)((v & 0xff00u) != 0u) << 1) | ((unsigned)((v & 0xff0000u) != 0u) << 2) |
           ((unsigned)((v & 0xff000000u) != 0u) << 3);
}
GS2M_DEVICE unsigned mask_nz16(const unsigned char* p) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    return mask_nz4(v.x) | (mask_nz4(v.y) << 4) | (mask_nz4(v.z) << 8) | (mask_nz4(v.w) << 12);
}
// byte i = bit i of m (4 bits -> 4 bytes of 0 / 1)
GS2M_DEVICE unsigned mask_bytes4(unsigned m) {
    return (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
}
// k_mask_pack with one thread per word (up to four 16-byte loads)
GS2M_KERNEL void __launch_bounds__(256)
k_mask_pack16(MaskBatch B, int W, int H, int nw, int invert, unsigned long long* __restrict__ bits) {
    const int f = (int)blockIdx.y;
    const unsigned char* obj = B.obj[f];
    if (!obj) return;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)H * nw) return;
    const int y = (int)(g / nw), w = (int)(g - (long long)y * nw);
    const int x0 = 64 * w, n16 = (W - x0) >= 64 ? 4 : (W - x0) >> 4;
    const unsigned char* r = obj + (size_t)y * W + x0;
    unsigned long long word = 0ull;
    for (int q = 0; q < n16; ++q) word |= (unsigned long long)mask_nz16(r + 16 * q) << (16 * q);
    if (invert) word = ~word & (n16 == 4 ? ~0ull : (1ull << (16 * n16)) - 1ull);
    mask_row(bits, f, H, nw, y)[w] = word;
}
// k_mask_output with one thread per 16 pixels
GS2M_KERNEL void __launch_bounds__(256)
k_mask_output16(MaskBatch B, int W, int H, int nw, int invert, const unsigned long long* __restrict__ bits) {
    const int f = (int)blockIdx.y;
    unsigned char* out = B.out[f];
    if (!out) return;
    const int cw = W >> 4;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= (long long)cw * H) return;
    const int y = (int)(c / cw), x0 = 16 * (int)(c - (long long)y * cw);
    const size_t p = (size_t)y * W + x0;
    const unsigned char* obj = B.obj[f];
    const unsigned char* occ = B.occ[f];
    unsigned m = 0xffffu;                                            // bit i = pixel x0 + i
    if (obj) {
        if (bits) m = ~(unsigned)(bits[((size_t)f * H + y) * nw + (x0 >> 6)] >> (x0 & 63)) & 0xffffu;
        else m = mask_nz16(obj + p) ^ (invert ? 0xffffu : 0u);
    }
    if (occ) m &= mask_nz16(occ + p);
    uint4 o;
    o.x = mask_bytes4(m);
    o.y = mask_bytes4(m >> 4);
    o.z = mask_bytes4(m >> 8);
    o.w = mask_bytes4(m >> 12);
    *reinterpret_cast<uint4*>(out + p) = o;
}

// one chunk of <= GS2M_MASK_BATCH frames.  a_bits / b_bits: [nf][H][nw] words each (unused without morphology).
static inline void gs2m_launch_mask_preprocess(hipStream_t st, const MaskBatch& B, int nf, int W, int H, int invert, int erode,
                                               int closing_k, int erosion_k, unsigned long long* a_bits, unsigned long long* b_bits) {
    const int nw = (W + 63) / 64;
    const long long words = (long long)H * nw;
    unsigned morph = 0u;
    bool vec = (W & 15) == 0;                                        // the 16-pixel forms: rows of whole 16-byte aligned chunks
    for (int f = 0; f < nf; ++f) {
        if (erode && B.obj[f]) morph |= 1u << f;
        vec = vec && ((uintptr_t)B.obj[f] & 15u) == 0 && ((uintptr_t)B.occ[f] & 15u) == 0 && ((uintptr_t)B.out[f] & 15u) == 0;
    }
    if (morph) {
        // the window offsets, clipped to the image (a wider window covers the same pixels)
        const int big = W > H ? W : H;
        int a1 = closing_k / 2, b1 = closing_k - 1 - closing_k / 2, a2 = erosion_k / 2, b2 = erosion_k - 1 - erosion_k / 2;
        a1 = a1 < big ? a1 : big;
        b1 = b1 < big ? b1 : big;
        a2 = a2 < big ? a2 : big;
        b2 = b2 < big ? b2 : big;
        const int k1 = a1 + b1 + 1, k2 = a2 + b2 + 1;
        const dim3 gw((unsigned)((words + 3) / 4), (unsigned)nf), gt((unsigned)((words + 255) / 256), (unsigned)nf);
        if (vec) GS2M_LAUNCH(k_mask_pack16, gt, dim3(256), 0, st, B, W, H, nw, invert, a_bits);
        else GS2M_LAUNCH(k_mask_pack, gw, dim3(256), 0, st, B, W, H, nw, invert, a_bits);
        GS2M_LAUNCH(k_mask_dilate_rows, gt, dim3(256), 0, st, morph, W, H, nw, a1, k1, 0, a_bits, b_bits);
        GS2M_LAUNCH(k_mask_dilate_cols, gt, dim3(256), 0, st, morph, H, nw, a1, b1, b_bits, a_bits);      // d1
        GS2M_LAUNCH(k_mask_dilate_rows, gt, dim3(256), 0, st, morph, W, H, nw, a1, k1, 1, a_bits, b_bits);
        GS2M_LAUNCH(k_mask_dilate_cols, gt, dim3(256), 0, st, morph, H, nw, a1, b1, b_bits, a_bits);      // d2 = ~closing
        GS2M_LAUNCH(k_mask_dilate_rows, gt, dim3(256), 0, st, morph, W, H, nw, a2, k2, 0, a_bits, b_bits);
        GS2M_LAUNCH(k_mask_dilate_cols, gt, dim3(256), 0, st, morph, H, nw, a2, b2, b_bits, a_bits);      // d3 = ~result
    }
    const unsigned long long* obits = morph ? (const unsigned long long*)a_bits : (const unsigned long long*)nullptr;
    if (vec)
        GS2M_LAUNCH(k_mask_output16, dim3((unsigned)(((long long)(W >> 4) * H + 255) / 256), (unsigned)nf), dim3(256), 0, st, B, W, H, nw,
                    invert, obits);
    else
        GS2M_LAUNCH(k_mask_output, dim3((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)nf), dim3(256), 0, st, B, W, H, nw, invert,
                    obits);
}
