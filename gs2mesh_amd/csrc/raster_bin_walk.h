// raster_bin_walk.h -- the walk of a Gaussian's tile rect, stated once for k_count_tiles and k_scatter (raster_project.h).
//
// The counting pass expands every rect into (Gaussian, tile) pairs and sizes the tile ranges; the scatter pass must visit exactly
// the same pairs to fill them.  Both therefore take every step of the walk from here: the class of a rect (bin_rect_class), the
// flattened item space of the staged rects (BinItems, bin_items_build, bin_item, bin_item_tile), the whole-wave walk of a rect of
// more than 64 tiles (bin_wave_begin, bin_wave_tile), the row-major cursor of a rect walked by its own lane (BinLaneCursor) and the
// prologue of the two kernels (bin_prologue, bin_row, bin_stage).  A kernel adds what it does with a tile: bump a histogram, or claim a slot and store a key.
#pragma once
#include "raster_math.h"

// ---- which rects of the binning grid get what ------------------------------------------------------------------------------
// cull = GS2M_OPT_EXACT_TILE_CULL: 0 = every tile of the (reference) rect is an instance; 1 = the rect is the bounding box of the
// alpha >= 1/255 ellipse and every tile of a rect with corners (>= 2 x 2 tiles) is tested against the ellipse; 2 (round 6) = the
// same, but rects of at most 4 tiles keep all their tiles -- the test only removes ~2 % of the instances of a small-splat
// scene (C3: 3.85 M -> 3.77 M per eye) and was 60 % of the vector instructions of the counting kernel, which is VALU-issue-bound
// (PMC round 5: 12 k vector instructions per wave, 0.8 of the SIMD's issue slots).  Rects of more than 64 tiles are walked by the
// whole wave and test every tile.  A thin rect (one tile wide or high) is its own bounding box: never tested.
GS2M_DEVICE bool gs2m_rect_tested(unsigned w, unsigned h, unsigned area, int cull) {
    return cull != 0 && (area > 64u || (w >= 2u && h >= 2u && (cull == 1 || area > 4u)));
}
// A rect of the binning grid that is one tile wide or one tile high and has at most GS2M_THIN_MAX tiles (round 4).
#define GS2M_THIN_MAX 4u
GS2M_DEVICE bool gs2m_thin_rect(unsigned w, unsigned h, unsigned area) {
    return area != 0u && area <= GS2M_THIN_MAX && (w == 1u || h == 1u);
}
// Rects that may be walked by THEIR OWN LANE (no staging, no item space): the thin ones and, round 6, every rect of at most
// `lane_max` tiles (GS2M_OPT_BIN_LANE_TILES).
#define GS2M_LANE_TILES_MAX 16
GS2M_DEVICE bool gs2m_lane_rect(unsigned w, unsigned h, unsigned area, unsigned lane_max) {
    return area != 0u && (area <= lane_max || gs2m_thin_rect(w, h, area));
}

// The class of a rect: exactly one of lane / staged / wave for a rect with tiles, none for an empty one.
//   lane   -- walked by its own lane (BinLaneCursor);
//   staged -- at most 64 tiles: an owner of the flattened item space (BinItems);
//   wave   -- more than 64 tiles: walked by the whole wave (bin_wave_begin, bin_wave_tile);
//   tested -- its tiles are tested against the ellipse, so a kept-tile mask exists for a staged or lane rect.
// `counting` is the ONE intended difference between the passes: k_count_tiles does not let a lane walk a tested rect -- the test
// costs ~35 vector instructions per tile, and a lane running it 4 times in sequence lost to the staged walk, which spreads the
// tiles over the lanes (measured, round 6) -- while k_scatter replays the mask the counting pass wrote, a bit test per tile.  The
// pairs visited are the same either way; only who visits them differs.
// The flags are WORD-sized on purpose.  Four `bool`s come back from the function packed into one register and are picked apart
// with byte operations: k_scatter<1 | 2> then had 7 | 13 instructions and an SGPR more than the two-copy form, and with the
// compiler's other answer to that shape k_count_tiles measured slower (profiles/binning_one_walk.txt).
struct BinClass {
    int lane, staged, wave, tested;   // 0 / 1
};
GS2M_DEVICE BinClass bin_rect_class(unsigned w, unsigned h, unsigned area, int cull, unsigned lane_max, bool counting) {
    BinClass c;
    c.tested = gs2m_rect_tested(w, h, area, cull);
    c.lane = !(counting && c.tested) && gs2m_lane_rect(w, h, area, lane_max);
    c.staged = area != 0u && area <= 64u && !c.lane;
    c.wave = area > 64u;
    return c;
}

GS2M_DEVICE unsigned long long lanes_le(int lane) { return (2ull << lane) - 1ull; }
GS2M_DEVICE unsigned long long lanes_lt(int lane) { return (1ull << lane) - 1ull; }

// li -> (rx, ry) of a rect of width ow without an integer division (li < 2^16, exact after one fix-up)
GS2M_DEVICE void rect_coords(unsigned li, unsigned ow, float inv_w, unsigned& rx, unsigned& ry) {
    ry = (unsigned)((float)li * inv_w);
    int r = (int)li - (int)(ry * ow);
    if (r < 0) {
        ry -= 1u;
        r += (int)ow;
    } else if (r >= (int)ow) {
        ry += 1u;
        r -= (int)ow;
    }
    rx = (unsigned)r;
}

GS2M_DEVICE unsigned wave_inclusive_scan(unsigned x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = gs2m_shfl_up(x, d);
        if (gs2m_lane() >= d) x += y;
    }
    return x;
}

// Gaussian -> workgroup assignment of the counting sort (the histogram row of a workgroup describes exactly the Gaussians it
// scatters).  Step `it` of wave `wave` of the workgroup with histogram row `row` starts at the returned index (64 consecutive
// Gaussians, one per lane); *end = one past the last index it may take; returns -1 when the wave is done.
//   contiguous (models in their stored order): the workgroup owns [row * chunk, (row + 1) * chunk) and walks it
//     blockDim.x Gaussians at a time;
//   interleaved (spatially ordered packed model, gs2m_raster_pack_model): blocks of 64 consecutive Gaussians are dealt
//     round-robin to the rows.  A block is a compact screen region (its instances fall into a few tiles: the keys of a
//     store instruction form runs), while every workgroup samples the whole model, so the work stays balanced (contiguous
//     chunks of a Morton-ordered model differ by 2.4x in instances on C2).
GS2M_DEVICE int bin_step_begin(int it, int wave, int nwaves, int row, int n_wg, int chunk, int P, int interleave, int* end) {
    if (interleave) {
        const long long first = (((long long)it * nwaves + wave) * n_wg + row) * 64ll;
        *end = P;
        return first < (long long)P ? (int)first : -1;
    }
    const int stop = gs2m_imin(P, (row + 1) * chunk);   // chunk <= 64000, rows < 2^15: no overflow
    const long long first = (long long)row * chunk + ((long long)it * nwaves + wave) * 64ll;
    *end = stop;
    return first < (long long)stop ? (int)first : -1;
}

// The tile rect of a record's binning part (16 x 16 tile units) in the binning grid (tiles of 16 x 16 * 2^rs pixels): rs = 0 / 1
// (a shift: the signed divisions by `rows` this replaces were ~100 of the ~800 vector instructions of a C3 counting step).
struct BinRect {
    int x0, y0;
    unsigned w, h, area;
};
GS2M_DEVICE BinRect bin_rect_of(const float4& c, int rs) {
    const unsigned rect0 = __float_as_uint(c.z), rect1 = __float_as_uint(c.w);
    const int x0 = (int)(rect0 & 0xffffu), x1 = (int)(rect1 & 0xffffu);
    const int y0 = (int)(rect0 >> 16), y1 = (int)(rect1 >> 16);
    const bool ok = x1 > x0 && y1 > y0;
    BinRect r;
    r.x0 = x0;
    r.y0 = y0 >> rs;
    r.w = ok ? (unsigned)(x1 - x0) : 0u;
    r.h = ok ? (unsigned)(((y1 + (1 << rs) - 1) >> rs) - r.y0) : 0u;
    r.area = r.w * r.h;
    return r;
}

// ---- prologue of the two kernels --------------------------------------------------------------------------------------------
// What a counting / scatter workgroup knows before its waves step through their Gaussians.
struct BinGrid {
    int gx, th, rs;      // binning grid: width in tiles, tile height in pixels, rows = 1 / 2 -> shift 0 / 1
    int tiles;
    unsigned lane_max;   // GS2M_OPT_BIN_LANE_TILES
    int cull;            // GS2M_OPT_EXACT_TILE_CULL
};
// Reads the grid and MOVES the caller's cams, recs, tilemask and hist to the group of NV views of this workgroup (blockIdx.y,
// GS2M_OPT_PAIR_BATCH): its own cameras, records, masks and histogram rows.
template <int NV, class Mask, class Hist>
GS2M_DEVICE BinGrid bin_prologue(const CamUniform* __restrict__& cams, GeomRecs& recs, int P, int n_wg, Mask* __restrict__& tilemask,
                                 Hist* __restrict__& hist, int exact_cull, int lane_tiles) {
    BinGrid g;
    g.gx = cams[0].gx;
    g.th = cams[0].th;
    g.rs = GS2M_CAM_ROWS(cams[0]) >> 1;
    g.tiles = g.gx * GS2M_CAM_GYS(cams[0]);
    g.lane_max = (unsigned)gs2m_uniform(lane_tiles);
    g.cull = gs2m_uniform(exact_cull);
    cams += NV * blockIdx.y;
    recs = gs2m_recs_at(recs, (size_t)NV * blockIdx.y * P);
    tilemask += (size_t)NV * blockIdx.y * P;
    hist += (size_t)NV * blockIdx.y * n_wg * g.tiles;
    return g;
}
// Histogram row = chunk of Gaussians of this workgroup.  The workgroups of one XCD own consecutive rows, so the segments an XCD
// writes into a tile are adjacent: its 8-B key stores fill whole lines in ITS L2 instead of leaving 1/8-written lines in eight
// L2s (4x write amplification, PMC WRITE_SIZE).  (Apart from bin_prologue: a scalar division that k_count_tiles does behind its
// barrier and k_scatter in front of its cursor loads, as before.)
GS2M_DEVICE int bin_row(int n_wg) { return (int)gs2m_xcd_contiguous(blockIdx.x, (unsigned)n_wg); }
// The dynamic LDS holds one u32 per (view, tile) -- the histogram of k_count_tiles, the cursors of k_scatter -- and behind it one
// Stage per wave; this is wave `wave`'s.  (Returned on its own: as a member of BinGrid the pointer cost k_count_tiles a second
// branch around the staging of a tested owner's geometry.)
template <int NV, class Stage>
GS2M_DEVICE Stage* bin_stage(unsigned* lds, int tiles, int wave) { return reinterpret_cast<Stage*>(lds + ((NV * tiles + 3) & ~3)) + wave; }

// ---- rects walked by their own lane: row-major walk with a running tile index (no multiplication per tile) ---------------------
struct BinLaneCursor {
    int tile;       // index of the current tile in the binning grid
    unsigned rx;    // its column inside the rect
};
GS2M_DEVICE BinLaneCursor bin_lane_begin(int x0, int y0, int gx) { return BinLaneCursor{y0 * gx + x0, 0u}; }
GS2M_DEVICE void bin_lane_next(BinLaneCursor& c, unsigned w, int gx) {
    ++c.tile;
    if (++c.rx == w) {
        c.rx = 0u;
        c.tile += gx - (int)w;
    }
}

// ---- wave-balanced tile expansion --------------------------------------------------------------------------------------------
// Every Gaussian touches a different number of tiles (1 ... hundreds).  Walking the rect per lane
// (as duplicateWithKeys does, rasterizer_impl.cu:98-108) leaves most lanes idle while the wave waits for
// its largest rect (C2: mean 8.6 tiles, mean of the per-wave maximum 38).  Instead:
//   * the owners of staged rects (<= 64 tiles) are compacted (rank k by ballot) and an exclusive wave scan
//     of their areas flattens all their (Gaussian, tile) pairs into one item space of <= 4096 items;
//   * a bit array marks the first item of every owner ("heads"); lane l of batch b0 takes item b0 + l and
//     finds its owner as  k = (#heads before the batch) + popcount(heads_word & lanes <= l) - 1
//     -- one broadcast LDS read and a popcount instead of a binary search;
//   * rects of more than 64 tiles (rare) are walked by the whole wave, one owner at a time.
// The kept tiles of a tested staged rect are a bit mask, row-major: assembled by the counting pass, replayed by the scatter.
struct BinItems {               // per wave, indexed by owner rank k
    unsigned swh[64];           // first item (16 bits) | w << 16 | h << 23 | tested << 31  (w, h <= 64: 7 bits each)
    unsigned xy0[64];           // x0 | y0 << 16
    unsigned mlo[64], mhi[64];  // kept-tile mask of the owner's rect
    unsigned heads[130];        // bit i: item i is the first item of an owner (+ slack for the 64-bit window)
    unsigned pad[2];
};
#define GS2M_BIN_TESTED 0x80000000u

// Builds the item space of one wave step (wave collective: EVERY lane calls it).  `staged`: this lane owns a staged rect (w, h,
// area, xy0, tested) whose mask starts as `mask`; `stageds` = the ballot of `staged`.  own(k) writes the kernel's own per-owner
// fields.  Returns the number of items; k = this lane's rank among the owners.
template <class Own>
GS2M_DEVICE unsigned bin_items_build(BinItems* it, int lane, bool staged, unsigned long long stageds, unsigned w, unsigned h,
                                     unsigned area, unsigned xy0, bool tested, unsigned long long mask, int& k, const Own own) {
    k = gs2m_popc64(stageds & lanes_lt(lane));
    const unsigned incl = wave_inclusive_scan(staged ? area : 0u);
    const unsigned total = gs2m_shfl(incl, 63);
    const unsigned start = incl - (staged ? area : 0u);
    gs2m_wave_sync();
    it->heads[lane] = 0u;
    it->heads[lane + 64] = 0u;
    if (lane < 2) it->heads[128 + lane] = 0u;
    gs2m_wave_sync();
    if (staged) {
        own(k);
        it->swh[k] = start | (w << 16) | (h << 23) | (tested ? GS2M_BIN_TESTED : 0u);
        it->xy0[k] = xy0;
        it->mlo[k] = (unsigned)mask;
        it->mhi[k] = (unsigned)(mask >> 32);
        atomicOr(&it->heads[start >> 5], 1u << (start & 31u));
    }
    gs2m_wave_sync();
    return total;
}

// This lane's item of the batch of 64 items that starts at b0 (wave collective).  kbase = owners before the batch: 0 at b0 = 0,
// carried by the caller from batch to batch in ascending order.  found(m) runs in the lanes whose item exists and says whether
// the kernel keeps the item's tile.  (A value the callable RETURNS: a flag it set through a reference capture cost the counting
// kernel six scalar instructions per batch and two SGPRs against the loop written in place.)
struct BinItem {
    unsigned long long H;   // head bits of the batch's items
    int kk;                 // rank of the item's owner
    bool act;               // the item exists; swh and li only then
    bool kept;              // ... and found() kept its tile
    unsigned swh;           // the owner's word
    unsigned li;            // row-major index of the item's tile inside the owner's rect
};
template <class Found>
GS2M_DEVICE BinItem bin_item(const BinItems* it, unsigned b0, unsigned total, int lane, int& kbase, const Found found) {
    BinItem m;
    m.H = (unsigned long long)it->heads[b0 >> 5] | ((unsigned long long)it->heads[(b0 >> 5) + 1] << 32);
    m.kk = kbase + gs2m_popc64(m.H & lanes_le(lane)) - 1;
    kbase += gs2m_popc64(m.H);
    const unsigned item = b0 + (unsigned)lane;
    m.act = item < total;
    m.swh = 0u;
    m.li = 0u;
    m.kept = false;
    if (m.act) {
        m.swh = it->swh[m.kk];
        m.li = item - (m.swh & 0xffffu);
        m.kept = found(m);
    }
    return m;
}
// (tx, ty) of an existing item in the binning grid.  Apart from bin_item: the scatter only asks for the items its mask keeps.
GS2M_DEVICE void bin_item_tile(const BinItems* it, const BinItem& m, int& tx, int& ty) {
    const unsigned ow = (m.swh >> 16) & 0x7fu;
    unsigned rx, ry;
    rect_coords(m.li, ow, gs2m_fast_rcp((float)ow), rx, ry);
    const unsigned oxy = it->xy0[m.kk];
    tx = (int)(oxy & 0xffffu) + (int)rx;
    ty = (int)(oxy >> 16) + (int)ry;
}

// One rect of more than 64 tiles, walked by the whole wave: lane l takes the tiles l, l + 64, ... of the rect.
//   const BinWave ww = bin_wave_begin(ow, oxy, geometry);                       wave-uniform: the owner's width, corner, geometry
//   for (unsigned li = lane; li < oa; li += 64u) { int tile; if (bin_wave_tile(ww, li, cull, gx, th, tile)) <keep tile>; }
// The loop stays in the kernel: handed over as a callable, the loop body moved the exit block of k_count_tiles' owner loop.
struct BinGeom {
    float mx, my, ca, cb, cc, thr;   // read only where the tiles are tested (cull != 0)
};
struct BinWave {
    unsigned ow, oxy;
    float oinv, srx, sry;
    BinGeom g;
};
GS2M_DEVICE BinWave bin_wave_begin(unsigned ow, unsigned oxy, const BinGeom& g) {
    BinWave ww;
    ww.ow = ow;
    ww.oxy = oxy;
    ww.g = g;
    ww.oinv = gs2m_fast_rcp((float)ow);
    cull_slopes(g.ca, g.cb, g.cc, ww.srx, ww.sry);
    return ww;
}
// tile = grid index of the rect's tile li (row-major); returns whether the rect keeps it
GS2M_DEVICE bool bin_wave_tile(const BinWave& ww, unsigned li, int cull, int gx, int th, int& tile) {
    unsigned rx, ry;
    rect_coords(li, ww.ow, ww.oinv, rx, ry);
    const int tx = (int)(ww.oxy & 0xffffu) + (int)rx, ty = (int)(ww.oxy >> 16) + (int)ry;
    tile = ty * gx + tx;
    return !cull || tile_may_contribute(ww.g.mx, ww.g.my, ww.g.ca, ww.g.cb, ww.g.cc, ww.srx, ww.sry, ww.g.thr, tx, ty, th);
}
