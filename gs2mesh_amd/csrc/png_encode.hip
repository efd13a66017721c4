// png_encode.hip -- device PNG encoder for the Renderer's left.png / right.png (files written
// asynchronously).  The stream is one a GPU produces in parallel and every zlib decodes:
//
//   8-bit RGB (colour type 2), no interlace; chunks IHDR, ONE IDAT, IEND.  zlib header 78 01.
//   Filtered scanlines (filter byte + 3W bytes per row; Paeth = type 4 on every row, or type 0) cut into segments of
//   S rows.  Each segment is ONE deflate block with its own dynamic Huffman code, literals only (HLIT 257, one distance
//   code of length 0: RFC 1951 3.2.7), literal lengths <= 15 bits, code-length lengths <= 7 bits, followed by an empty
//   stored block (zlib's sync flush), so every segment starts on a byte boundary and is written independently.  A
//   segment whose dynamic form is not smaller than storing it is stored instead (blocks of <= 65535 bytes, already
//   byte-aligned).  The stream ends with an empty final fixed block (03 00) and the Adler-32 of the filtered scanlines.
//   Output bytes depend only on the pixels, S and the filter (integer arithmetic throughout).
//
// Five launches per call, all on the caller's stream, no host read:
//   k_png_codes     one workgroup per (image, segment): filter, 257-bin histogram, Adler partials; one lane builds the
//                   length-limited code (Moffat-Katajainen lengths, Kraft repair), the run-length coded tree header and
//                   the exact size of the dynamic form; decides dynamic / stored.  The filtered bytes are not kept:
//                   k_png_encode recomputes them from the pixels (no scratch round trip of 5.8 MB per image).
//   k_png_assemble  one workgroup per image: exclusive scan of the segment sizes, the fixed parts of the file
//                   (signature, IHDR + CRC, IDAT length, zlib header, 03 00, Adler-32, IEND), the file size.
//   k_png_encode    one workgroup per (image, segment): the segment's bits written straight into the caller's output
//                   at its scanned offset.  Per round each lane codes 16 bytes; a workgroup scan gives the bit offsets;
//                   the lanes OR their bits into an LDS staging buffer; whole words go out with one store each (the
//                   first / last word of a segment byte by byte: they share bytes with the neighbours).
//   k_png_crc_chunks + k_png_crc_finish   CRC-32 of the IDAT chunk: 16 KiB chunks of the assembled bytes, combined with
//                   zlib's crc32_combine arithmetic (multiplication by x^(8 len) mod P).  The chunking is aligned at the
//                   END of the range (leading zero bytes leave a zero-initialised CRC at zero), so every piece that is
//                   combined is a power of two bytes long and every shift is one entry of the x^(2^k) table.
#include <stdint.h>
#include <string.h>

#include "../../include/gs2mesh_amd.h"
#include "platform.h"

#define PNG_THREADS 256
#define PNG_WAVES (PNG_THREADS / 64)
#define PNG_CHUNK 16                          // filtered bytes per lane per round of k_png_encode
#define PNG_ROUND (PNG_THREADS * PNG_CHUNK)   // 4096
#define PNG_SYMS 257                          // 256 literals + end-of-block
#define PNG_CODE_STRIDE 260                   // words per segment in the code table scratch
#define PNG_HDR_WORDS 128                     // tree header <= 17 + 19 * 3 + 258 * 14 = 3686 bits
#define PNG_STAGE_WORDS 2112                  // one round (4096 x 15 bits) + 31 carried bits + end-of-block, in words
#define PNG_CRC_SPAN 64                       // bytes per lane of k_png_crc_chunks (2^6)
#define PNG_CRC_CHUNK (PNG_THREADS * PNG_CRC_SPAN)   // 16 KiB = 2^14
#define PNG_PREFIX 43                         // signature 8 + IHDR 25 + IDAT length / type 8 + zlib header 2
#define PNG_FIXED 65                          // PNG_PREFIX + 03 00 + Adler 4 + IDAT CRC 4 + IEND 12
#define PNG_MAX_SEGMENT (1 << 28)             // bytes of one segment: keeps sum(i * b) of the Adler partials in 64 bits
#define PNG_STORED_BLOCK 65535u
#define PNG_ADLER_MOD 65521ull
#define PNG_CRC_POLY 0xedb88320u

struct PngSeg {                 // k_png_codes -> k_png_assemble / k_png_encode
    unsigned bytes;             // encoded size of the segment (dynamic block + sync flush, or stored blocks)
    unsigned dynamic;           // 1 = dynamic Huffman block, 0 = stored
    unsigned hdr_bits;          // bits of the block header (BFINAL/BTYPE, HLIT/HDIST/HCLEN, code-length code, lengths)
    unsigned pad;
    unsigned long long s0, s1;  // Adler partials: sum b, sum i*b (i = position in the segment)
};

struct PngImg {                 // k_png_assemble -> the CRC kernels
    unsigned long long idat_len;
    unsigned long long total;
};

// ---- shared helpers ------------------------------------------------------------------------------------------------
GS2M_DEVICE unsigned png_min_u(unsigned a, unsigned b) { return a < b ? a : b; }

// filtered byte x (0 .. 3W-1) of image row `row` (pixels `img`, row pitch rb = 3W bytes)
GS2M_DEVICE unsigned png_filt(const unsigned char* img, int rb, int row, int x, int filter) {
    const unsigned char* cur = img + (size_t)row * rb;
    const int v = cur[x];
    if (filter == 0) return (unsigned)v;
    const int a = x >= 3 ? cur[x - 3] : 0;
    const int b = row > 0 ? cur[x - rb] : 0;
    const int c = (row > 0 && x >= 3) ? cur[x - rb - 3] : 0;
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return (unsigned)(v - pred) & 255u;
}

// byte `col` (0 = the filter-type byte) of the filtered scanline of image row `row`
GS2M_DEVICE unsigned png_stream_byte(const unsigned char* img, int rb, int row, int col, int filter) {
    return col == 0 ? (unsigned)filter : png_filt(img, rb, row, col - 1, filter);
}

GS2M_DEVICE unsigned png_stored_bytes(unsigned L) { return L + 5u * ((L + PNG_STORED_BLOCK - 1u) / PNG_STORED_BLOCK); }

// a * b modulo the CRC-32 polynomial (reflected bit order, as zlib's multmodp)
GS2M_DEVICE unsigned png_multmodp(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}

// Moffat-Katajainen in place: A[0..n) = frequencies in ascending order -> A[i] = Huffman code length of entry i
GS2M_DEVICE void png_mk_lengths(unsigned* A, int n) {
    if (n == 1) {
        A[0] = 1;
        return;
    }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (unsigned)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (unsigned)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, depth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == depth) {
            ++used;
            --root;
        }
        while (avbl > used) {
            A[next--] = (unsigned)depth;
            --avbl;
        }
        avbl = 2 * used;
        ++depth;
        used = 0;
    }
}

// code lengths <= maxb for the n symbols order[0..n) (ascending frequency; the frequencies in A on entry, clobbered)
// -> lens[sym].  Lengths over maxb are clamped, then leaves move down until the Kraft sum is exactly 1 (complete code).
GS2M_DEVICE void png_limited_lengths(unsigned* A, const unsigned short* order, int n, int maxb, unsigned char* lens,
                                     int* blc) {
    png_mk_lengths(A, n);
    for (int l = 0; l <= maxb; ++l) blc[l] = 0;
    for (int i = 0; i < n; ++i) blc[A[i] > (unsigned)maxb ? maxb : (int)A[i]]++;
    unsigned total = 0;
    for (int l = 1; l <= maxb; ++l) total += (unsigned)blc[l] << (maxb - l);
    while (total > (1u << maxb)) {
        blc[maxb]--;
        for (int l = maxb - 1; l > 0; --l) {
            if (blc[l]) {
                blc[l]--;
                blc[l + 1] += 2;
                break;
            }
        }
        total--;
    }
    int i = 0;
    for (int l = maxb; l >= 1; --l)
        for (int k = 0; k < blc[l]; ++k) lens[order[i++]] = (unsigned char)l;
}

GS2M_DEVICE unsigned png_reverse(unsigned code, int len) {
    unsigned r = 0;
    for (int k = 0; k < len; ++k) r = (r << 1) | ((code >> k) & 1u);
    return r;
}

// code-length alphabet order of the HCLEN field (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
GS2M_DEVICE int png_cl_perm(int i) {
    switch (i) {
        case 0: return 16;  case 1: return 17;  case 2: return 18;  case 3: return 0;   case 4: return 8;
        case 5: return 7;   case 6: return 9;   case 7: return 6;   case 8: return 10;  case 9: return 5;
        case 10: return 11; case 11: return 4;  case 12: return 12; case 13: return 3;  case 14: return 13;
        case 15: return 2;  case 16: return 14; case 17: return 1;  default: return 15;
    }
}

// serial LSB-first bit writer into a zeroed word array
GS2M_DEVICE void png_put_bits(unsigned* w, unsigned& pos, unsigned v, int n) {
    if (n == 0) return;
    const unsigned sh = pos & 31u;
    w[pos >> 5] |= v << sh;
    if (sh + (unsigned)n > 32u) w[(pos >> 5) + 1] |= v >> (32u - sh);
    pos += (unsigned)n;
}

// ---- pass 1: filter + histogram + Adler partials, then the segment's code (one lane) ------------------------------
GS2M_KERNEL void __launch_bounds__(PNG_THREADS)
k_png_codes(const unsigned char* __restrict__ rgb, long long img_stride, int W, int H, int S, int filter, int nseg,
            PngSeg* __restrict__ segs, unsigned* __restrict__ codes, unsigned* __restrict__ hdr) {
    __shared__ unsigned hist[PNG_SYMS];
    __shared__ unsigned A[PNG_SYMS];
    __shared__ unsigned short order[PNG_SYMS];
    __shared__ unsigned char lens[PNG_SYMS + 1];     // + the one distance code (length 0)
    __shared__ unsigned next_code[16];
    __shared__ int blc[16];
    __shared__ unsigned char rle_sym[PNG_SYMS + 1], rle_ext[PNG_SYMS + 1];
    __shared__ unsigned cl_freq[19];
    __shared__ unsigned cl_code[19];
    __shared__ unsigned short cl_order[19];
    __shared__ unsigned char cl_len[19];
    __shared__ unsigned hw[PNG_HDR_WORDS];
    __shared__ unsigned long long red0[PNG_WAVES], red1[PNG_WAVES];
    __shared__ unsigned dyn_flag;

    const int tid = (int)threadIdx.x;
    const int seg = (int)blockIdx.x, img = (int)blockIdx.y;
    const int id = img * nseg + seg;
    const unsigned char* im = rgb + (size_t)img * (size_t)img_stride;
    const int rb = 3 * W;
    const unsigned R = (unsigned)rb + 1u;
    const int r0 = seg * S;
    const int rows = H - r0 < S ? H - r0 : S;
    const unsigned L = (unsigned)rows * R;

    for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) hist[s] = s == PNG_SYMS - 1 ? 1u : 0u;   // end-of-block once
    for (int s = tid; s < PNG_HDR_WORDS; s += PNG_THREADS) hw[s] = 0u;
    __syncthreads();

    unsigned long long s0 = 0, s1 = 0;
    for (unsigned base = (unsigned)tid * PNG_CHUNK; base < L; base += PNG_ROUND) {
        const unsigned end = png_min_u(base + PNG_CHUNK, L);
        int row = r0 + (int)(base / R);
        int col = (int)(base % R);
        unsigned run_v = 0u, run_n = 0u;
        for (unsigned i = base; i < end; ++i) {
            const unsigned v = png_stream_byte(im, rb, row, col, filter);
            s0 += v;
            s1 += (unsigned long long)i * v;
            if (v != run_v && run_n) {   // flat runs cost one LDS atomic, not one per byte
                atomicAdd(&hist[run_v], run_n);
                run_n = 0u;
            }
            run_v = v;
            ++run_n;
            if (++col == (int)R) {
                col = 0;
                ++row;
            }
        }
        if (run_n) atomicAdd(&hist[run_v], run_n);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += gs2m_shfl_xor(s0, d);
        s1 += gs2m_shfl_xor(s1, d);
    }
    if (gs2m_lane() == 0) {
        red0[tid >> 6] = s0;
        red1[tid >> 6] = s1;
    }
    __syncthreads();

    // symbols in ascending (frequency, symbol) order: rank of each present symbol among the present ones
    for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) {
        const unsigned f = hist[s];
        if (f) {
            int rank = 0;
            for (int u = 0; u < PNG_SYMS; ++u) {
                const unsigned g = hist[u];
                rank += (g != 0u && (g < f || (g == f && u < s))) ? 1 : 0;
            }
            order[rank] = (unsigned short)s;
        }
        lens[s] = 0;
    }
    const int n = gs2m_syncthreads_count(hist[tid] != 0u) + 1;   // literals present + end-of-block

    if (tid == 0) {
        // ---- literal/length code: lengths <= 15 -----------------------------------------------------------------------
        lens[PNG_SYMS] = 0;
        for (int i = 0; i < n; ++i) A[i] = hist[order[i]];
        png_limited_lengths(A, order, n, 15, lens, blc);
        unsigned long long data_bits = 0;
        for (int s = 0; s < PNG_SYMS; ++s) data_bits += (unsigned long long)hist[s] * lens[s];
        // canonical code bases (RFC 1951 3.2.2)
        for (int l = 0; l < 16; ++l) blc[l] = 0;
        for (int s = 0; s < PNG_SYMS; ++s) blc[lens[s]]++;
        blc[0] = 0;
        unsigned code = 0;
        for (int l = 1; l < 16; ++l) {
            code = (code + (unsigned)blc[l - 1]) << 1;
            next_code[l] = code;
        }
        // ---- run-length coded lengths: 257 literal/length + 1 distance, one sequence ---------------------------------
        int m = 0;
        for (int c = 0; c < 19; ++c) cl_freq[c] = 0;
        for (int i = 0; i < PNG_SYMS + 1;) {
            const unsigned v = lens[i];
            int run = 1;
            while (i + run < PNG_SYMS + 1 && lens[i + run] == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const int k = run < 138 ? run : 138;
                    rle_sym[m] = 18;
                    rle_ext[m++] = (unsigned char)(k - 11);
                    run -= k;
                }
                if (run >= 3) {
                    rle_sym[m] = 17;
                    rle_ext[m++] = (unsigned char)(run - 3);
                    run = 0;
                }
                for (; run > 0; --run) rle_sym[m++] = 0;
            } else {
                rle_sym[m++] = (unsigned char)v;
                --run;
                while (run >= 3) {
                    const int k = run < 6 ? run : 6;
                    rle_sym[m] = 16;
                    rle_ext[m++] = (unsigned char)(k - 3);
                    run -= k;
                }
                for (; run > 0; --run) rle_sym[m++] = (unsigned char)v;
            }
        }
        for (int j = 0; j < m; ++j) cl_freq[rle_sym[j]]++;
        // ---- code-length code: lengths <= 7 (insertion sort of <= 19 symbols) ---------------------------------------
        int n2 = 0;
        for (int c = 0; c < 19; ++c) {
            cl_len[c] = 0;
            if (!cl_freq[c]) continue;
            int j = n2++;
            while (j > 0 && cl_freq[cl_order[j - 1]] > cl_freq[c]) {
                cl_order[j] = cl_order[j - 1];
                --j;
            }
            cl_order[j] = (unsigned short)c;
        }
        if (n2 == 1) {   // a one-symbol code is incomplete for inflate: give a second (unused) symbol a code too
            cl_order[1] = cl_order[0];
            cl_order[0] = (unsigned short)(cl_order[1] == 0 ? 1 : 0);
            n2 = 2;
        }
        for (int i = 0; i < n2; ++i) A[i] = cl_freq[cl_order[i]];
        png_limited_lengths(A, cl_order, n2, 7, cl_len, blc);
        for (int l = 0; l < 8; ++l) blc[l] = 0;
        for (int c = 0; c < 19; ++c) blc[cl_len[c]]++;
        blc[0] = 0;
        unsigned cc = 0;
        for (int l = 1; l < 8; ++l) {
            cc = (cc + (unsigned)blc[l - 1]) << 1;
            blc[8 + l] = (int)cc;   // next code of length l
        }
        for (int c = 0; c < 19; ++c) {
            const int l = cl_len[c];
            cl_code[c] = l ? png_reverse((unsigned)blc[8 + l]++, l) : 0u;
        }
        // ---- block header ---------------------------------------------------------------------------------------------
        int hclen = 19;
        while (hclen > 4 && cl_len[png_cl_perm(hclen - 1)] == 0) --hclen;
        unsigned pos = 0;
        png_put_bits(hw, pos, 4u, 3);                 // BFINAL 0, BTYPE 2 (dynamic)
        png_put_bits(hw, pos, 0u, 5);                 // HLIT - 257
        png_put_bits(hw, pos, 0u, 5);                 // HDIST - 1
        png_put_bits(hw, pos, (unsigned)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) png_put_bits(hw, pos, cl_len[png_cl_perm(i)], 3);
        for (int j = 0; j < m; ++j) {
            const int c = rle_sym[j];
            png_put_bits(hw, pos, cl_code[c], cl_len[c]);
            if (c == 16) png_put_bits(hw, pos, rle_ext[j], 2);
            else if (c == 17) png_put_bits(hw, pos, rle_ext[j], 3);
            else if (c == 18) png_put_bits(hw, pos, rle_ext[j], 7);
        }
        const unsigned long long bits = pos + data_bits;
        const unsigned long long dyn_bytes = (bits + 3ull + 7ull) / 8ull + 4ull;   // + empty stored block (sync flush)
        const unsigned stored = png_stored_bytes(L);
        const unsigned dyn = dyn_bytes < (unsigned long long)stored ? 1u : 0u;
        dyn_flag = dyn;
        PngSeg info;
        info.bytes = dyn ? (unsigned)dyn_bytes : stored;
        info.dynamic = dyn;
        info.hdr_bits = pos;
        info.pad = 0u;
        info.s0 = red0[0] + red0[1] + red0[2] + red0[3];
        info.s1 = red1[0] + red1[1] + red1[2] + red1[3];
        segs[id] = info;
    }
    __syncthreads();
    if (!dyn_flag) return;
    // canonical, bit-reversed codes: code(s) = next_code[len] + #{u < s : len(u) == len}
    for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) {
        const int l = lens[s];
        unsigned word = 0u;
        if (l) {
            unsigned k = 0;
            for (int u = 0; u < s; ++u) k += lens[u] == l ? 1u : 0u;
            word = png_reverse(next_code[l] + k, l) | ((unsigned)l << 16);
        }
        codes[(size_t)id * PNG_CODE_STRIDE + s] = word;
    }
    for (int w = tid; w < PNG_HDR_WORDS; w += PNG_THREADS) hdr[(size_t)id * PNG_HDR_WORDS + w] = hw[w];
}

// ---- pass 2: offsets + the fixed parts of the file (one workgroup per image) ----------------------------------------
GS2M_DEVICE void png_put_be32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)(v >> 24);
    p[1] = (unsigned char)(v >> 16);
    p[2] = (unsigned char)(v >> 8);
    p[3] = (unsigned char)v;
}

GS2M_KERNEL void __launch_bounds__(PNG_THREADS)
k_png_assemble(int W, int H, int S, int nseg, const PngSeg* __restrict__ segs, unsigned long long* __restrict__ seg_off,
               PngImg* __restrict__ imgs, const unsigned* __restrict__ crc_tab, unsigned char* __restrict__ out,
               long long out_stride, long long* __restrict__ out_bytes) {
    __shared__ unsigned long long wtot[PNG_WAVES];
    __shared__ unsigned long long wad[PNG_WAVES];
    const int tid = (int)threadIdx.x, lane = gs2m_lane(), wave = tid >> 6;
    const int img = (int)blockIdx.x;
    const unsigned long long R = 3ull * (unsigned long long)W + 1ull;
    const unsigned long long n_raw = R * (unsigned long long)H;
    unsigned long long base = PNG_PREFIX;
    unsigned long long adler_b = 0, adler_a = 0;   // this lane's segments' shares, mod 65521
    for (int c = 0; c < nseg; c += PNG_THREADS) {
        const int s = c + tid;
        unsigned long long v = 0;
        if (s < nseg) {
            const PngSeg sg = segs[(size_t)img * nseg + s];
            v = sg.bytes;
            // B = n + sum_i (n - i) b_i over the whole stream; a segment starting at `start` adds (n - start) s0 - s1
            const unsigned long long start = (unsigned long long)s * (unsigned long long)S * R;
            adler_a = (adler_a + sg.s0 % PNG_ADLER_MOD) % PNG_ADLER_MOD;
            const unsigned long long t = ((n_raw - start) % PNG_ADLER_MOD) * (sg.s0 % PNG_ADLER_MOD) % PNG_ADLER_MOD;
            adler_b = (adler_b + t + PNG_ADLER_MOD - sg.s1 % PNG_ADLER_MOD) % PNG_ADLER_MOD;
        }
        unsigned long long x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = gs2m_shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (int w = 0; w < PNG_WAVES; ++w) {
            before += w < wave ? wtot[w] : 0ull;
            all += wtot[w];
        }
        if (s < nseg) seg_off[(size_t)img * nseg + s] = base + before + x - v;
        base += all;
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) {
        adler_a += gs2m_shfl_xor(adler_a, d);
        adler_b += gs2m_shfl_xor(adler_b, d);
    }
    if (lane == 0) {
        wtot[wave] = adler_a;
        wad[wave] = adler_b;
    }
    __syncthreads();
    if (tid != 0) return;
    unsigned long long a = 1, b = n_raw % PNG_ADLER_MOD;
    for (int w = 0; w < PNG_WAVES; ++w) {
        a += wtot[w];
        b += wad[w];
    }
    a %= PNG_ADLER_MOD;
    b %= PNG_ADLER_MOD;
    const unsigned long long seg_total = base - PNG_PREFIX;
    const unsigned long long idat_len = 2ull + seg_total + 2ull + 4ull;
    const unsigned long long total = seg_total + PNG_FIXED;
    unsigned char* o = out + (size_t)img * (size_t)out_stride;
    o[0] = 0x89; o[1] = 'P'; o[2] = 'N'; o[3] = 'G'; o[4] = 0x0d; o[5] = 0x0a; o[6] = 0x1a; o[7] = 0x0a;
    png_put_be32(o + 8, 13u);
    o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
    png_put_be32(o + 16, (unsigned)W);
    png_put_be32(o + 20, (unsigned)H);
    o[24] = 8;   // bit depth
    o[25] = 2;   // colour type: RGB
    o[26] = 0;   // compression
    o[27] = 0;   // filter method
    o[28] = 0;   // interlace
    unsigned crc = 0xffffffffu;
    for (int i = 12; i < 29; ++i) crc = crc_tab[(crc ^ o[i]) & 255u] ^ (crc >> 8);
    png_put_be32(o + 29, ~crc);
    png_put_be32(o + 33, (unsigned)idat_len);
    o[37] = 'I'; o[38] = 'D'; o[39] = 'A'; o[40] = 'T';
    o[41] = 0x78;   // zlib: deflate, 32 KiB window
    o[42] = 0x01;   // FLEVEL 0, no dictionary, FCHECK
    unsigned char* t = o + base;
    t[0] = 0x03;    // final fixed block holding only end-of-block
    t[1] = 0x00;
    png_put_be32(t + 2, (unsigned)((b << 16) | a));
    // t + 6: IDAT CRC (k_png_crc_finish), then IEND
    png_put_be32(t + 10, 0u);
    t[14] = 'I'; t[15] = 'E'; t[16] = 'N'; t[17] = 'D';
    png_put_be32(t + 18, 0xae426082u);
    PngImg info;
    info.idat_len = idat_len;
    info.total = total;
    imgs[img] = info;
    out_bytes[img] = (long long)total;
}

// ---- pass 3: the segment's bits, straight into the file ------------------------------------------------------------
// store of 4 bytes at the 4-aligned address `a`, of which only [lo, hi) belong to this segment
GS2M_DEVICE void png_put_word(unsigned char* a, unsigned v, const unsigned char* lo, const unsigned char* hi) {
    if (a >= lo && a + 4 <= hi) {
        *reinterpret_cast<unsigned*>(a) = v;
        return;
    }
    for (int j = 0; j < 4; ++j)
        if (a + j >= lo && a + j < hi) a[j] = (unsigned char)(v >> (8 * j));
}

// every lane: write the whole words pending in the stage and clear them; the partial word becomes word 0
GS2M_DEVICE void png_flush(unsigned* stage, unsigned& carry, unsigned char*& gbase, const unsigned char* lo,
                           const unsigned char* hi, int tid) {
    const unsigned nfull = carry >> 5;
    for (unsigned w = (unsigned)tid; w < nfull; w += PNG_THREADS) {
        png_put_word(gbase + 4u * w, stage[w], lo, hi);
        stage[w] = 0u;
    }
    __syncthreads();
    if (nfull) {
        if (tid == 0) {
            stage[0] = stage[nfull];
            stage[nfull] = 0u;
        }
        gbase += 4u * nfull;
        carry &= 31u;
    }
}

GS2M_KERNEL void __launch_bounds__(PNG_THREADS)
k_png_encode(const unsigned char* __restrict__ rgb, long long img_stride, int W, int H, int S, int filter, int nseg,
             const PngSeg* __restrict__ segs, const unsigned* __restrict__ codes, const unsigned* __restrict__ hdr,
             const unsigned long long* __restrict__ seg_off, unsigned char* __restrict__ out, long long out_stride) {
    __shared__ unsigned cw[PNG_SYMS];
    __shared__ unsigned stage[PNG_STAGE_WORDS];
    __shared__ unsigned wtot[PNG_WAVES];
    const int tid = (int)threadIdx.x, lane = gs2m_lane(), wave = tid >> 6;
    const int seg = (int)blockIdx.x, img = (int)blockIdx.y;
    const int id = img * nseg + seg;
    const unsigned char* im = rgb + (size_t)img * (size_t)img_stride;
    const int rb = 3 * W;
    const unsigned R = (unsigned)rb + 1u;
    const int r0 = seg * S;
    const int rows = H - r0 < S ? H - r0 : S;
    const unsigned L = (unsigned)rows * R;
    const PngSeg sg = segs[id];
    unsigned char* dst = out + (size_t)img * (size_t)out_stride + seg_off[id];

    if (!sg.dynamic) {   // stored blocks: 00, LEN, NLEN (little-endian), then up to 65535 filtered bytes
        for (unsigned p = (unsigned)tid; p < sg.bytes; p += PNG_THREADS) {
            const unsigned blk = p / (PNG_STORED_BLOCK + 5u), q = p - blk * (PNG_STORED_BLOCK + 5u);
            unsigned v;
            if (q < 5u) {
                const unsigned len = png_min_u(PNG_STORED_BLOCK, L - blk * PNG_STORED_BLOCK);
                const unsigned h = q < 3u ? len : ~len;
                v = q == 0u ? 0u : (h >> (((q - 1u) & 1u) ? 8 : 0)) & 255u;
            } else {
                const unsigned i = blk * PNG_STORED_BLOCK + q - 5u;
                v = png_stream_byte(im, rb, r0 + (int)(i / R), (int)(i % R), filter);
            }
            dst[p] = (unsigned char)v;
        }
        return;
    }

    for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) cw[s] = codes[(size_t)id * PNG_CODE_STRIDE + s];
    for (int w = tid; w < PNG_STAGE_WORDS; w += PNG_THREADS) stage[w] = 0u;
    const unsigned shift = (unsigned)((uintptr_t)dst & 3u);
    unsigned char* gbase = dst - shift;    // 4-aligned; stage bit 0 = bit 0 of this address
    const unsigned char* const lo = dst;
    const unsigned char* const hi = dst + sg.bytes;
    __syncthreads();
    // block header at stage bit 8 * shift (the bytes below belong to the previous segment and are never written)
    for (int w = tid; w < PNG_HDR_WORDS; w += PNG_THREADS) {
        const unsigned v = hdr[(size_t)id * PNG_HDR_WORDS + w];
        if (v) {
            const unsigned sh = 8u * shift;
            atomicOr(&stage[w], v << sh);
            if (sh) atomicOr(&stage[w + 1], v >> (32u - sh));
        }
    }
    unsigned carry = 8u * shift + sg.hdr_bits;   // bits pending in the stage, from bit 0 of word 0
    __syncthreads();

    for (unsigned rpos = 0; rpos < L; rpos += PNG_ROUND) {
        png_flush(stage, carry, gbase, lo, hi, tid);
        // code this lane's 16 bytes, scan the bit counts over the workgroup
        const unsigned base = rpos + (unsigned)tid * PNG_CHUNK;
        unsigned cword[PNG_CHUNK];
        unsigned nb = 0;
        {
            int row = r0 + (int)(base / R);
            int col = (int)(base % R);
#pragma unroll
            for (int k = 0; k < PNG_CHUNK; ++k) {
                unsigned c = 0u;
                if (base + (unsigned)k < L) {
                    c = cw[png_stream_byte(im, rb, row, col, filter)];
                    if (++col == (int)R) {
                        col = 0;
                        ++row;
                    }
                }
                cword[k] = c;
                nb += c >> 16;
            }
        }
        unsigned x = nb;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = gs2m_shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < PNG_WAVES; ++w) {
            before += w < wave ? wtot[w] : 0u;
            all += wtot[w];
        }
        // OR the bits into the stage (only the words shared with the neighbouring lanes actually collide)
        {
            const unsigned p0 = carry + before + x - nb;
            unsigned word = p0 >> 5;
            unsigned fill = p0 & 31u;
            unsigned long long acc = 0ull;
#pragma unroll
            for (int k = 0; k < PNG_CHUNK; ++k) {
                acc |= (unsigned long long)(cword[k] & 0xffffu) << fill;
                fill += cword[k] >> 16;
                if (fill >= 32u) {
                    atomicOr(&stage[word], (unsigned)acc);
                    acc >>= 32;
                    fill -= 32u;
                    ++word;
                }
            }
            if (fill) atomicOr(&stage[word], (unsigned)acc);
        }
        carry += all;
        __syncthreads();
    }
    png_flush(stage, carry, gbase, lo, hi, tid);
    // end-of-block, then the sync flush: 3 zero bits, pad to the byte, 00 00 ff ff
    if (tid == 0) {
        const unsigned e = cw[PNG_SYMS - 1];
        const unsigned len = e >> 16;
        const unsigned sh = carry & 31u;
        stage[carry >> 5] |= (e & 0xffffu) << sh;
        if (sh + len > 32u) stage[(carry >> 5) + 1] |= (e & 0xffffu) >> (32u - sh);
        carry += len;
        const unsigned nbytes = (carry + 3u + 7u) >> 3;
        for (unsigned j = 0; j < nbytes; ++j) {
            unsigned char* a = gbase + j;
            if (a >= lo && a < hi) *a = (unsigned char)(stage[j >> 2] >> (8u * (j & 3u)));
        }
        unsigned char* t = gbase + nbytes;
        for (int j = 0; j < 4; ++j)
            if (t + j >= lo && t + j < hi) t[j] = j < 2 ? 0x00 : 0xff;
    }
}

// ---- pass 4: IDAT CRC-32 ---------------------------------------------------------------------------------------------
// CRC register of the chunk type + data, zero-initialised (no pre / post inversion: linear in the bytes)
GS2M_KERNEL void __launch_bounds__(PNG_THREADS)
k_png_crc_chunks(const PngImg* __restrict__ imgs, const unsigned* __restrict__ tabs, const unsigned char* __restrict__ out,
                 long long out_stride, unsigned* __restrict__ chunk_crc, int max_chunks) {
    __shared__ unsigned tab[256];
    __shared__ unsigned part[PNG_THREADS];
    const int tid = (int)threadIdx.x;
    const int img = (int)blockIdx.y;
    const unsigned long long N = 4ull + imgs[img].idat_len;   // "IDAT" + data
    const unsigned long long nch = (N + PNG_CRC_CHUNK - 1) / PNG_CRC_CHUNK;
    const unsigned long long pad = nch * PNG_CRC_CHUNK - N;    // virtual leading zero bytes
    const unsigned long long c = blockIdx.x;
    if (c >= nch) return;
    const unsigned* x2n = tabs + 256;
    tab[tid] = tabs[tid];
    __syncthreads();
    const unsigned char* src = out + (size_t)img * (size_t)out_stride + 37;
    const unsigned long long v0 = c * PNG_CRC_CHUNK + (unsigned long long)tid * PNG_CRC_SPAN;
    unsigned crc = 0u;
    for (int k = 0; k < PNG_CRC_SPAN; ++k) {
        const unsigned long long v = v0 + (unsigned long long)k;
        if (v >= pad) crc = tab[(crc ^ src[v - pad]) & 255u] ^ (crc >> 8);
    }
    for (int j = 0; (1 << j) < PNG_THREADS; ++j) {   // pieces of 2^(6 + j) bytes: shift by x^(2^(9 + j))
        part[tid] = crc;
        __syncthreads();
        const int s = 1 << j;
        if ((tid & (2 * s - 1)) == 0) crc = png_multmodp(x2n[9 + j], crc) ^ part[tid + s];
        __syncthreads();
    }
    if (tid == 0) chunk_crc[(size_t)img * max_chunks + c] = crc;
}

GS2M_KERNEL void __launch_bounds__(PNG_THREADS)
k_png_crc_finish(const PngImg* __restrict__ imgs, const unsigned* __restrict__ tabs, const unsigned* __restrict__ chunk_crc,
                 int max_chunks, unsigned char* __restrict__ out, long long out_stride) {
    __shared__ unsigned part[PNG_THREADS];
    const int tid = (int)threadIdx.x;
    const int img = (int)blockIdx.x;
    const unsigned* x2n = tabs + 256;
    const unsigned long long idat_len = imgs[img].idat_len;
    const unsigned long long N = 4ull + idat_len;
    const unsigned nch = (unsigned)((N + PNG_CRC_CHUNK - 1) / PNG_CRC_CHUNK);
    int lk = 0;   // chunks per lane = 2^lk; the padded chunk count 256 * 2^lk (leading zero chunks)
    while (((unsigned)PNG_THREADS << lk) < nch) ++lk;
    const unsigned k = 1u << lk;
    const unsigned padc = ((unsigned)PNG_THREADS << lk) - nch;
    unsigned crc = 0u;
    for (unsigned j = 0; j < k; ++j) {
        const unsigned vc = (unsigned)tid * k + j;
        const unsigned cc = vc >= padc ? chunk_crc[(size_t)img * max_chunks + (vc - padc)] : 0u;
        crc = png_multmodp(x2n[17], crc) ^ cc;                 // 2^14-byte chunks: x^(2^17)
    }
    for (int j = 0; (1 << j) < PNG_THREADS; ++j) {
        part[tid] = crc;
        __syncthreads();
        const int s = 1 << j;
        if ((tid & (2 * s - 1)) == 0) crc = png_multmodp(x2n[(17 + lk + j) & 31], crc) ^ part[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    // standard CRC-32 = ~(register of the bytes from 0  ^  register 0xffffffff carried over N bytes)
    unsigned xn = 0x80000000u;   // x^0
    unsigned long long m = N;
    for (int b = 3; m; m >>= 1, ++b)
        if (m & 1ull) xn = png_multmodp(x2n[b & 31], xn);
    const unsigned v = ~(crc ^ png_multmodp(xn, 0xffffffffu));
    png_put_be32(out + (size_t)img * (size_t)out_stride + 41 + idat_len, v);
}

// ---- host ------------------------------------------------------------------------------------------------------------
#include "device_memory.h"

struct gs2m_png {
    int device = 0;
    DeviceBuffer<unsigned> d_tabs;   // [256] CRC-32 byte table, [32] x^(2^k) mod P
    ScratchArena arena;              // per-call temporaries, grow-only
};

static unsigned host_multmodp(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}

extern "C" int gs2m_png_create(gs2m_png** out, int device) {
    if (!out) {
        gs2m_set_error("gs2m_png_create: out is NULL");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(device));
    unsigned tabs[256 + 32];
    for (unsigned n = 0; n < 256; ++n) {
        unsigned c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PNG_CRC_POLY : c >> 1;
        tabs[n] = c;
    }
    unsigned x = 1u << 30;   // x^1
    tabs[256] = x;
    for (int k = 1; k < 32; ++k) tabs[256 + k] = x = host_multmodp(x, x);
    gs2m_png* h = new gs2m_png();
    h->device = device;
    if (h->d_tabs.reserve_exact(256 + 32) ||
        hipMemcpy(h->d_tabs.get(), tabs, sizeof(tabs), hipMemcpyHostToDevice) != hipSuccess) {
        gs2m_set_error("gs2m_png_create: allocation failed");
        delete h;
        return 1;
    }
    *out = h;
    return 0;
}

extern "C" int gs2m_png_destroy(gs2m_png* p) {
    if (!p) return 0;
    (void)hipSetDevice(p->device);
    delete p;   // the table and the arena are members
    return 0;
}

static int64_t png_stored_bound(int64_t L) { return L + 5 * ((L + PNG_STORED_BLOCK - 1) / PNG_STORED_BLOCK); }

extern "C" int64_t gs2m_png_max_bytes(int width, int height, int rows_per_segment) {
    if (width <= 0 || height <= 0 || rows_per_segment <= 0 || width > (1 << 26)) return -1;
    const int64_t R = 3 * (int64_t)width + 1;
    const int64_t S = rows_per_segment < height ? rows_per_segment : height;
    if (S * R > PNG_MAX_SEGMENT) return -1;
    const int64_t full = height / S, last = height % S;
    const int64_t total = PNG_FIXED + full * png_stored_bound(S * R) + (last ? png_stored_bound(last * R) : 0);
    if (total - 57 > (int64_t)0x7fffffff) return -1;   // the IDAT length is a 31-bit field
    return total;
}

extern "C" int gs2m_png_encode(gs2m_png* p, int n, int width, int height, const uint8_t* rgb8, int64_t image_stride,
                               uint8_t* out, int64_t out_stride, int64_t* out_bytes, int filter, int rows_per_segment,
                               gs2m_stream stream) {
    if (!p || n <= 0 || !rgb8 || !out || !out_bytes || (filter != 0 && filter != 4)) {
        gs2m_set_error("gs2m_png_encode: bad argument");
        return 1;
    }
    const int64_t max_bytes = gs2m_png_max_bytes(width, height, rows_per_segment);
    if (max_bytes < 0) {
        gs2m_set_error("gs2m_png_encode: unsupported size %d x %d, rows_per_segment %d", width, height, rows_per_segment);
        return 1;
    }
    if (out_stride < max_bytes) {
        gs2m_set_error("gs2m_png_encode: out_stride %lld < gs2m_png_max_bytes %lld", (long long)out_stride,
                       (long long)max_bytes);
        return 1;
    }
    if (n > 1 && image_stride < 3 * (int64_t)width * height) {
        gs2m_set_error("gs2m_png_encode: image_stride %lld < 3 * width * height", (long long)image_stride);
        return 1;
    }
    if (n > 65535) {
        gs2m_set_error("gs2m_png_encode: at most 65535 images per call");
        return 1;
    }
    const int S = rows_per_segment < height ? rows_per_segment : height;
    const int nseg = (height + S - 1) / S;
    const size_t nsegs = (size_t)n * nseg;
    const int max_chunks = (int)((max_bytes + PNG_CRC_CHUNK - 1) / PNG_CRC_CHUNK);
    PngSeg* segs;
    unsigned *codes, *hdr, *chunk_crc;
    unsigned long long* seg_off;
    PngImg* imgs;
    GS2M_HIPCHK(hipSetDevice(p->device));
    if (p->arena.carve(arena_sub(segs, nsegs), arena_sub(codes, nsegs * PNG_CODE_STRIDE), arena_sub(hdr, nsegs * PNG_HDR_WORDS),
                       arena_sub(seg_off, nsegs), arena_sub(imgs, (size_t)n), arena_sub(chunk_crc, (size_t)n * max_chunks)))
        return 1;
    const unsigned* tabs = p->d_tabs.get();
    const long long istride = (long long)image_stride, ostride = (long long)out_stride;
    GS2M_LAUNCH(k_png_codes, dim3(nseg, n), dim3(PNG_THREADS), 0, stream, rgb8, istride, width, height, S, filter, nseg,
                segs, codes, hdr);
    GS2M_LAUNCH(k_png_assemble, dim3(n), dim3(PNG_THREADS), 0, stream, width, height, S, nseg, (const PngSeg*)segs,
                seg_off, imgs, tabs, out, ostride, (long long*)out_bytes);
    GS2M_LAUNCH(k_png_encode, dim3(nseg, n), dim3(PNG_THREADS), 0, stream, rgb8, istride, width, height, S, filter, nseg,
                (const PngSeg*)segs, (const unsigned*)codes, (const unsigned*)hdr, (const unsigned long long*)seg_off, out,
                ostride);
    GS2M_LAUNCH(k_png_crc_chunks, dim3(max_chunks, n), dim3(PNG_THREADS), 0, stream, (const PngImg*)imgs, tabs,
                (const unsigned char*)out, ostride, chunk_crc, max_chunks);
    GS2M_LAUNCH(k_png_crc_finish, dim3(n), dim3(PNG_THREADS), 0, stream, (const PngImg*)imgs, tabs,
                (const unsigned*)chunk_crc, max_chunks, out, ostride);
    return 0;
}
