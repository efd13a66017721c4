// raster_project.h -- kernels of the projection / tile-counting / instance-scatter stages.
//
// Stage map (reference -> here):
//   preprocessCUDA            forward.cu:155-256          -> k_project (fused activations, Sigma once per
//                                                            Gaussian for all views of the batch)
//   cub InclusiveSum + D2H    rasterizer_impl.cu:277-281  -> k_count_tiles (per-workgroup LDS tile histogram
//   duplicateWithKeys         rasterizer_impl.cu:70-111      instead of a per-Gaussian scan)
//                                                         -> k_scatter (LDS cursors, 8-B keys)
// Instead of emitting (tile<<32|depth, id) pairs in Gaussian order and radix-sorting 64-bit keys
// through HBM 5-6 times, instances are counting-sorted by tile with workgroup-private LDS
// histograms (160 KiB LDS holds a 40k-tile cursor array), then depth-sorted per tile in
// registers (raster_sort.h).  The final order is identical to the reference's: ascending depth bits, ties
// by ascending Gaussian id (= what the stable radix sort over emission order produces).
#pragma once
#include "raster_bin_walk.h"

// Workgroup-private tile histogram of k_count_tiles: one u32 counter per (view, tile) in LDS.  (Rounds 2-5 packed two 16-bit
// counters per word to halve the LDS; the kernel runs one 1024-thread workgroup per CU either way -- the scatter kernel's u32
// cursors set the LDS budget of the pair -- and the hi / lo select cost 4 of the 6 vector instructions of a bump in a kernel that
// is vector-issue-bound.  Round 6 also measured, and dropped, wave-aggregated bumps (one atomic per run of neighbouring lanes
// with the same tile) and 2 / 4 lane-interleaved copies of the histogram against the same-address serialisation of a spatially
// ordered model's atomics: C3 count 29.7 -> 36.8 us (aggregated), 30.4 -> 29.6 (copies) -- profiles/r6_experiments.txt.)
GS2M_DEVICE void hist_bump(unsigned* hh, int t) { atomicAdd(&hh[t], 1u); }

struct ProjView {
    float mx, my, ca, cb, cc, depth, cova, covc;
    int x0, y0, x1, y1, radius;
    bool ok;
};

// Geometry of one Gaussian in one view: forward.cu:186-237 up to the zero-area test.
GS2M_DEVICE void project_view(const CamUniform& cam, float px, float py, float pz, const float* cov3, ProjView& o) {
    o.ok = false;
    o.radius = 0;
    o.x0 = o.y0 = o.x1 = o.y1 = 0;
    o.mx = o.my = o.ca = o.cb = o.cc = o.depth = o.cova = o.covc = 0.0f;
    float tvx, tvy, tvz;
    xform4x3(cam.view, px, py, pz, tvx, tvy, tvz);
    if (tvz <= 0.2f) return;  // auxiliary.h:154 near cull
    float hx, hy, hz, hw;
    xform4x4(cam.proj, px, py, pz, hx, hy, hz, hw);
    const float p_w = 1.0f / (hw + 0.0000001f);
    const float ppx = hx * p_w, ppy = hy * p_w;
    float a, b, c;
    cov2d_ewa(cam.view, tvx, tvy, tvz, cam.focal_x, cam.focal_y, cam.tanfovx, cam.tanfovy, cov3, a, b, c);
    const float det = (a * c - b * b);
    if (det == 0.0f) return;
    const float det_inv = 1.f / det;
    o.cova = a;
    o.covc = c;
    o.ca = c * det_inv;
    o.cb = -b * det_inv;
    o.cc = a * det_inv;
    const float mid = 0.5f * (a + c);
    const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
    const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
    o.mx = ndc2pix(ppx, cam.W);
    o.my = ndc2pix(ppy, cam.H);
    // Non-finite / overflowing input (DESIGN.md "Parity"): every float -> int below is gs2m_f2i_sat (NaN -> 0, saturating).
    const int r = gs2m_f2i_sat(my_radius);
    // auxiliary.h:46-56 getRect
    o.x0 = gs2m_imin(cam.gx, gs2m_imax(0, gs2m_f2i_sat((o.mx - r) / GS2M_TILE)));
    o.y0 = gs2m_imin(cam.gy, gs2m_imax(0, gs2m_f2i_sat((o.my - r) / GS2M_TILE)));
    o.x1 = gs2m_imin(cam.gx, gs2m_imax(0, gs2m_f2i_sat((o.mx + r + GS2M_TILE - 1) / GS2M_TILE)));
    o.y1 = gs2m_imin(cam.gy, gs2m_imax(0, gs2m_f2i_sat((o.my + r + GS2M_TILE - 1) / GS2M_TILE)));
    // r <= 0 (a NaN radius; the reference emits no instance for radii == 0, rasterizer_impl.cu:85): invisible, as radius 0 says
    if (r <= 0 || (o.x1 - o.x0) * (o.y1 - o.y0) == 0) {
        o.x0 = o.y0 = o.x1 = o.y1 = 0;
        return;
    }
    o.depth = tvz;
    o.radius = r;
    o.ok = true;
}

// Projection + colour, one thread per Gaussian -- a streaming kernel (no LDS, no loop): activations, Sigma once
// for all views of the batch, EWA projection, SH colour, the (cull-tightened) tile rect -> GeomRec.
#define GS2M_PROJECT_THREADS 256
// One Gaussian (array position gi) for the `groups` x NV views of the launch: parameter loads (+ fused activations) and Sigma
// ONCE, then per group of NV views (a stereo pair) the EWA projection, SH colour, the (cull-tightened) tile rect and the GeomRec
// stores.  Round 6: the groups of a launch (GS2M_OPT_PAIR_BATCH) used to be blockIdx.y -- every group re-read the 44 B of
// parameters and the 192-B SH row of every Gaussian, 71 % of the kernel's bytes; now the thread that owns the Gaussian walks the
// groups (LOOP), the row stays in LDS (DMA_SH) or is re-read through the caches (streamed path): C3 project 113.5 -> 86.5 us per
// pair.  The loop costs registers (84 -> 128, 106 -> 152: 4 -> 3 waves per SIMD on the streamed path) and halves the waves of the
// launch, and a model that fits the 256 MB last-level cache re-reads cheaply anyway (C2: 18.4 -> 19.5 us with the loop): the
// launcher keeps the groups on blockIdx.y (LOOP = false, `groups` = 1) for models below GS2M_PROJECT_LOOP_MIN_P Gaussians.
// s_sh = this wave's DMA landing zone, [12][64] float4 (DMA_SH only).
#define GS2M_PROJECT_LOOP_MIN_P 1000000
template <int NV, bool DMA_SH, bool STREAM = true, bool LOOP = false>
GS2M_DEVICE void project_gaussian(const GaussIn& g, const CamUniform* __restrict__ cams, GeomRecs recs,
                                  int* __restrict__ radii, int exact_cull, int gi, bool valid, float4* s_sh, int lane_id,
                                  int groups) {
    const int ncoef = (g.D + 1) * (g.D + 1);
    constexpr bool dma_sh = DMA_SH;
    {
        if (dma_sh && valid) {
            const float4* s4 = reinterpret_cast<const float4*>(g.shs_packed) + (size_t)(gi >> 6) * (12 * 64) + (gi & 63);
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k * 4 < ncoef * 3) gs2m_global_load_lds16(s4 + k * 64, &s_sh[k * 64]);
        }
        if (valid) {
            const float px = g.xyz[3 * (size_t)gi], py = g.xyz[3 * (size_t)gi + 1], pz = g.xyz[3 * (size_t)gi + 2];
            float cov3[6];
            if (g.cov3D_precomp) {
#pragma unroll
                for (int k = 0; k < 6; ++k) cov3[k] = g.cov3D_precomp[6 * (size_t)gi + k];
            } else {
                float sx = g.scales[3 * (size_t)gi], sy = g.scales[3 * (size_t)gi + 1], sz = g.scales[3 * (size_t)gi + 2];
                const float4 q4 = *reinterpret_cast<const float4*>(g.rots + 4 * (size_t)gi);
                float qr = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
                if (g.raw) {
                    // GaussianModel getters (GS/scene/gaussian_model.py:95-101): exp, F.normalize
                    sx = expf(sx);
                    sy = expf(sy);
                    sz = expf(sz);
                    const float n = fmaxf(sqrtf(qr * qr + qx * qx + qy * qy + qz * qz), 1e-12f);
                    qr = qr / n;
                    qx = qx / n;
                    qy = qy / n;
                    qz = qz / n;
                }
                cov3d_from_scale_rot(sx, sy, sz, g.scale_modifier, qr, qx, qy, qz, cov3);
            }
            float op = g.opac[gi];
            if (g.raw) op = 1.0f / (1.0f + expf(-op));  // gaussian_model.py:113-115 sigmoid
            const float thr = exact_cull ? cull_threshold(op) : 0.0f;
            const CamUniform* __restrict__ cams0 = cams;
            const GeomRecs recs0 = recs;
            int* __restrict__ const radii0 = radii;
#pragma unroll 1
            for (int grp = 0; grp < (LOOP ? groups : 1); ++grp) {
            cams = cams0 + NV * grp;
            recs = gs2m_recs_at(recs0, (size_t)NV * grp * g.P);
            radii = radii0 ? radii0 + (size_t)NV * grp * g.P : nullptr;
            // the SH row is loop-invariant: re-read it per group (LDS / caches) instead of letting the compiler hoist 48 registers
            // of it over the loop (4 -> 3 waves per SIMD)
            int gi_sh = gi, lane_sh = lane_id;
            if (LOOP) {
                GS2M_OPAQUE_VGPR(gi_sh);
                GS2M_OPAQUE_VGPR(lane_sh);
            }
            ProjView pv[NV];
            bool any = false;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                project_view(cams[v], px, py, pz, cov3, pv[v]);
                any = any || pv[v].ok;
            }
            // colour: the 192-B SH row is STREAMED for all views at once where it is 16-B aligned (packed copy, [P,16,3] or
            // the DMA landing zone): three float4 in flight instead of 48 registers for the row.  dc + rest split layouts
            // and M != 16 keep the register path below.
            // STREAM (chosen by the launcher from the layout) compiles the 48-register path out.
            const bool stream_sh = STREAM && (g.colors_precomp == nullptr) && (dma_sh || g.shs_packed != nullptr || (g.shs_rest == nullptr && g.M == 16));
            float rgb_v[NV][3];
#pragma unroll
            for (int v = 0; v < NV; ++v) rgb_v[v][0] = rgb_v[v][1] = rgb_v[v][2] = 0.0f;
            if (dma_sh && grp == 0) gs2m_wait_dma();   // this lane's row has landed (a lane only reads its own column: no barrier)
            if (stream_sh && any && !dma_sh) {
                float dirs[NV][3];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    // forward.cu:25-27: dir = (pos - campos) / length
                    float dx = px - cams[v].campos[0], dy = py - cams[v].campos[1], dz = pz - cams[v].campos[2];
                    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
                    dirs[v][0] = dx / len;
                    dirs[v][1] = dy / len;
                    dirs[v][2] = dz / len;
                }
                if (g.shs_packed) {
                    // wave-transposed copy (k_pack_sh): float4 j of 64 consecutive Gaussians is 1 KiB contiguous
                    const float4* s4 = reinterpret_cast<const float4*>(g.shs_packed) + (size_t)(gi_sh >> 6) * (12 * 64) + (gi_sh & 63);
                    sh_rgb_stream<NV>(g.D, [&](int j) { return s4[j * 64]; }, dirs, rgb_v);
                } else {
                    const float4* s4 = reinterpret_cast<const float4*>(g.shs + 48 * (size_t)gi_sh);   // 192-B row, 16-B aligned
                    sh_rgb_stream<NV>(g.D, [&](int j) { return s4[j]; }, dirs, rgb_v);
                }
            }
            float sh[STREAM ? 1 : 48];
            const bool need_sh = !STREAM && any && (g.colors_precomp == nullptr) && !stream_sh;
            if constexpr (!STREAM) if (need_sh) {
                if (g.shs_rest == nullptr) {
                    const float* s = g.shs + (size_t)gi_sh * g.M * 3;
#pragma unroll
                    for (int k = 0; k < 48; ++k)
                        if (k < ncoef * 3) sh[k] = s[k];
                } else {
                    const float* s0 = g.shs + (size_t)gi_sh * 3;
                    const float* s1 = g.shs_rest + (size_t)gi_sh * (g.M - 1) * 3;
                    sh[0] = s0[0];
                    sh[1] = s0[1];
                    sh[2] = s0[2];
#pragma unroll
                    for (int k = 3; k < 48; ++k)
                        if (k < ncoef * 3) sh[k] = s1[k - 3];
                }
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const size_t ri = (size_t)v * g.P + gi;
                if (radii) radii[(size_t)v * g.P + (g.ids ? g.ids[gi] : gi)] = pv[v].radius;
                if (!pv[v].ok) {
                    // invisible: only the vector holding the (empty) rect is written
                    float4 w2;
                    w2.x = 0.0f;
                    w2.y = 0.0f;
                    w2.z = 0.0f;
                    w2.w = 0.0f;
                    recs.c[ri] = w2;
                    continue;
                }
                float cr, cg, cb;
                if (g.colors_precomp) {
                    cr = g.colors_precomp[3 * (size_t)gi];
                    cg = g.colors_precomp[3 * (size_t)gi + 1];
                    cb = g.colors_precomp[3 * (size_t)gi + 2];
                } else if (dma_sh) {
                    // forward.cu:25-27: dir = (pos - campos) / length; the row is read back from LDS view by view
                    float dirs[1][3], col[1][3];
                    const float dx = px - cams[v].campos[0], dy = py - cams[v].campos[1], dz = pz - cams[v].campos[2];
                    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
                    dirs[0][0] = dx / len;
                    dirs[0][1] = dy / len;
                    dirs[0][2] = dz / len;
                    sh_rgb_stream<1>(g.D, [&](int j) { return s_sh[j * 64 + lane_sh]; }, dirs, col);
                    cr = col[0][0];
                    cg = col[0][1];
                    cb = col[0][2];
                } else if (stream_sh) {
                    cr = rgb_v[v][0];
                    cg = rgb_v[v][1];
                    cb = rgb_v[v][2];
                } else {
                    cr = cg = cb = 0.0f;
                    if constexpr (!STREAM) {
                        // forward.cu:25-27: dir = (pos - campos) / length
                        float dx = px - cams[v].campos[0], dy = py - cams[v].campos[1], dz = pz - cams[v].campos[2];
                        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
                        dx = dx / len;
                        dy = dy / len;
                        dz = dz / len;
                        cr = sh_channel(g.D, sh, 0, dx, dy, dz);
                        cg = sh_channel(g.D, sh, 1, dx, dy, dz);
                        cb = sh_channel(g.D, sh, 2, dx, dy, dz);
                    }
                }
                // GS2M_OPT_EXACT_TILE_CULL (image-preserving extension): shrink the reference's AABB-of-
                // the-3-sigma-circle rect to the bounding box of the alpha >= 1/255 ellipse,
                // |dx| <= sqrt(2 t cov_xx), |dy| <= sqrt(2 t cov_yy), t = ln(255 o) (+ margin).  The
                // stored rect is what the counting sort and the scatter walk.
                if (exact_cull) {
                    if (thr < 0.0f) {
                        pv[v].x1 = pv[v].x0 = pv[v].y0 = pv[v].y1 = 0;  // never reaches 1/255 anywhere
                    } else {
                        const float hx = sqrtf(2.0f * thr * pv[v].cova) + 0.01f;
                        const float hy = sqrtf(2.0f * thr * pv[v].covc) + 0.01f;
                        // the + 1 in float: exact wherever the box can bind (|tiles| < 2^24), and no int overflow at +inf
                        const int bx0 = gs2m_f2i_sat(ceilf((pv[v].mx - hx - (float)(GS2M_TILE - 1)) / GS2M_TILE));
                        const int bx1 = gs2m_f2i_sat(floorf((pv[v].mx + hx) / GS2M_TILE) + 1.0f);
                        const int by0 = gs2m_f2i_sat(ceilf((pv[v].my - hy - (float)(GS2M_TILE - 1)) / GS2M_TILE));
                        const int by1 = gs2m_f2i_sat(floorf((pv[v].my + hy) / GS2M_TILE) + 1.0f);
                        pv[v].x0 = gs2m_imax(pv[v].x0, bx0);
                        pv[v].y0 = gs2m_imax(pv[v].y0, by0);
                        pv[v].x1 = gs2m_imin(pv[v].x1, bx1);
                        pv[v].y1 = gs2m_imin(pv[v].y1, by1);
                        if (pv[v].x1 <= pv[v].x0 || pv[v].y1 <= pv[v].y0) pv[v].x1 = pv[v].x0 = pv[v].y0 = pv[v].y1 = 0;
                    }
                }
                float4 w0, w1, w2;
                w0.x = pv[v].mx;
                w0.y = pv[v].my;
                w0.z = pv[v].ca;
                w0.w = pv[v].cb;
                w1.x = pv[v].cc;
                w1.y = op;
                w1.z = cr;
                w1.w = cg;
                w2.x = cb;
                w2.y = pv[v].depth;
                w2.z = __uint_as_float((unsigned)pv[v].x0 | ((unsigned)pv[v].y0 << 16));
                w2.w = __uint_as_float((unsigned)pv[v].x1 | ((unsigned)pv[v].y1 << 16));
                recs.ab[2 * ri] = w0;
                recs.ab[2 * ri + 1] = w1;
                recs.c[ri] = w2;
            }
            }   // groups
        }
    }
}

// Per-view uniforms from HOST values carried in the kernel arguments (pipeline-level API): the launch packet is the
// transport, so no pinned staging buffer / lifetime hazard.  Round 4: the packet is k_project's own (its workgroups read the
// uniforms of their views straight from the kernel-argument segment -- scalar loads -- and workgroup 0 of every group of views
// stores them to `cams_out` for the later kernels of the pass): one launch less on the critical chain of every pass (round 3:
// k_set_cameras, 4.5 us + a launch gap).
struct CamUniformArg {
    CamUniform c[GS2M_MAX_PASS_VIEWS];
};

// Projection + colour, one thread per Gaussian -- a streaming kernel (no loop): see project_gaussian.
// Packed SH copy (DMA_SH): the 192-B row of every Gaussian of the wave goes straight from HBM into LDS (global_load_lds, 12 x
// 1 KiB per wave), issued BEFORE the parameter loads and the projection: one memory round trip per thread instead of two in
// sequence (the wave spent 69 % of its life waiting, PMC) and no 48 registers holding the row while it is in flight.  The
// colour pass then reads the 16 coefficients of one channel at a time back from LDS.
template <int NV, bool DMA_SH, bool STREAM, bool HOSTCAMS, bool LOOP>
GS2M_DEVICE void project_kernel_body(const GaussIn& g, const CamUniform* __restrict__ cams, GeomRecs recs,
                                     int* __restrict__ radii, int exact_cull, CamUniform* __restrict__ cams_out, int groups) {
    __shared__ float4 s_sh[DMA_SH ? GS2M_PROJECT_THREADS / 64 : 1][DMA_SH ? 12 : 1][DMA_SH ? 64 : 1];
    // the groups of NV views of the launch (GS2M_OPT_PAIR_BATCH: two stereo pairs per launch): LOOP -- all `groups` of them are
    // walked by the thread that owns the Gaussian (project_gaussian); else blockIdx.y = the group of this workgroup
    const int g0 = LOOP ? 0 : (int)blockIdx.y, ng = LOOP ? groups : 1;
    cams += NV * g0;
    if (HOSTCAMS && blockIdx.x == 0) {
        // the uniforms of this workgroup's views -> device memory, for the later kernels of the pass (dword copy)
        const unsigned* src = reinterpret_cast<const unsigned*>(cams);
        unsigned* dst = reinterpret_cast<unsigned*>(cams_out + NV * g0);
        for (unsigned i = threadIdx.x; i < (unsigned)(ng * NV) * (unsigned)(sizeof(CamUniform) / 4u); i += GS2M_PROJECT_THREADS) dst[i] = src[i];
    }
    recs = gs2m_recs_at(recs, (size_t)NV * g0 * g.P);
    if (radii) radii += (size_t)NV * g0 * g.P;
    const int gi = (int)(blockIdx.x * (unsigned)GS2M_PROJECT_THREADS + threadIdx.x);
    const int wave_id = (int)(threadIdx.x >> 6), lane_id = (int)(threadIdx.x & 63u);
    project_gaussian<NV, DMA_SH, STREAM, LOOP>(g, cams, recs, radii, exact_cull, gi, gi < g.P, &s_sh[DMA_SH ? wave_id : 0][0][0], lane_id, ng);
}
// uniforms in device memory (operator-level API: the caller's matrices are device tensors, k_pack_camera)
template <int NV, bool DMA_SH, bool STREAM = true, bool LOOP = false>
GS2M_KERNEL void __launch_bounds__(GS2M_PROJECT_THREADS)   // forcing 5 waves per SIMD on the round-2 kernel (96 VGPRs, spills): C2 30 -> 36 us, C3 149 -> 204
k_project(GaussIn g, const CamUniform* __restrict__ cams, GeomRecs recs, int* __restrict__ radii,
          int exact_cull, int groups) {
    project_kernel_body<NV, DMA_SH, STREAM, false, LOOP>(g, cams, recs, radii, exact_cull, nullptr, groups);
}
// uniforms in the kernel arguments (pipeline-level API, host-side cameras)
template <int NV, bool DMA_SH, bool STREAM = true, bool LOOP = false>
GS2M_KERNEL void __launch_bounds__(GS2M_PROJECT_THREADS)
k_project_hc(GaussIn g, CamUniformArg hc, CamUniform* __restrict__ cams_out, GeomRecs recs, int* __restrict__ radii,
             int exact_cull, int groups) {
    project_kernel_body<NV, DMA_SH, STREAM, true, LOOP>(g, &hc.c[0], recs, radii, exact_cull, cams_out, groups);
}

// Per-(view, Gaussian) input of the counting step: the geometry half of the GeomRec + the rect in BINNING rows.
struct CountIn {
    float mx, my, ca, cb, cc;
    int x0, y0, x1, y1;
    bool ok;
};
// Stage of a counting wave: the item space and, for its tested owners, what the tile test reads (indexed by owner rank k).
struct WaveStage {
    float mx[64], my[64], ca[64], cb[64], cc[64], thr[64], rx[64], ry[64];
    BinItems items;
};

// The counting step for the 64 Gaussians of one wave step (wave collectives: EVERY lane calls it): the walk of raster_bin_walk.h;
// each kept (Gaussian, tile) pair bumps the workgroup's LDS tile histogram, and the kept tiles of a tested staged rect are recorded
// as a bit mask (assembled from ballots by the first lane of each owner's run) that the scatter kernel replays.
template <int NV>
GS2M_DEVICE void count_expand(const CountIn* pv, float thr, bool valid, int gi, int P, unsigned* lhist, int tiles, WaveStage* stage,
                              unsigned long long* __restrict__ tilemask, int gx, int th, int cull, int lane, unsigned lane_max) {
    BinItems* const it = &stage->items;
#pragma unroll
    for (int v = 0; v < NV; ++v) {   // one view at a time
        const unsigned w = (unsigned)(pv[v].x1 - pv[v].x0), h = (unsigned)(pv[v].y1 - pv[v].y0);
        const unsigned area = (valid && pv[v].ok) ? w * h : 0u;
        if (gs2m_ballot(area != 0u ? 1 : 0) == 0ull) continue;  // wave-uniform
        unsigned* hh = lhist + v * tiles;
        const unsigned xy0 = (unsigned)pv[v].x0 | ((unsigned)pv[v].y0 << 16);
        const BinClass rc = bin_rect_class(w, h, area, cull, lane_max, true);
        // ---- rects walked by their own lane: thin ones (round 4) and untested ones of <= lane_max tiles (round 6).  Every tile
        // is kept: no staging, no item space, no tile mask.  A 2 M-Gaussian scene of small splats is 85 % thin + 14 % 2 x 2
        // rects (C3, 16 x 32 binning tiles).
        if (gs2m_ballot(rc.lane ? 1 : 0) != 0ull) {
            const unsigned area_l = rc.lane ? area : 0u;
            BinLaneCursor c = bin_lane_begin(pv[v].x0, pv[v].y0, gx);
            for (unsigned t = 0; t < area_l; ++t) {
                hist_bump(hh, c.tile);
                bin_lane_next(c, w, gx);
            }
        }
        // ---- the other rects of <= 64 tiles: flattened item space ----
        const unsigned long long stageds = gs2m_ballot(rc.staged ? 1 : 0);
        if (stageds != 0ull) {
            int k;
            const unsigned total = bin_items_build(it, lane, rc.staged, stageds, w, h, area, xy0, rc.tested, 0ull, k,
                                                   [&](int ko) __attribute__((always_inline)) {
                if (rc.tested) {
                    stage->mx[ko] = pv[v].mx;
                    stage->my[ko] = pv[v].my;
                    stage->ca[ko] = pv[v].ca;
                    stage->cb[ko] = pv[v].cb;
                    stage->cc[ko] = pv[v].cc;
                    stage->thr[ko] = thr;
                    cull_slopes(pv[v].ca, pv[v].cb, pv[v].cc, stage->rx[ko], stage->ry[ko]);
                }
            });
            int kbase = 0;
            for (unsigned b0 = 0; b0 < total; b0 += 64u) {
                const BinItem m = bin_item(it, b0, total, lane, kbase, [&](const BinItem& m) __attribute__((always_inline)) {
                    int tx, ty;
                    bin_item_tile(it, m, tx, ty);
                    bool keep = true;
                    if (m.swh & GS2M_BIN_TESTED)  // only tested rects (corners to cut)
                        keep = tile_may_contribute(stage->mx[m.kk], stage->my[m.kk], stage->ca[m.kk], stage->cb[m.kk],
                                                   stage->cc[m.kk], stage->rx[m.kk], stage->ry[m.kk], stage->thr[m.kk], tx, ty, th);
                    if (keep) hist_bump(hh, ty * gx + tx);
                    return keep;
                });
                // the first lane of each owner's run in this batch folds the run's keep bits into the owner's mask
                const unsigned long long kept = gs2m_ballot(m.kept ? 1 : 0);
                if (m.act && (lane == 0 || ((m.H >> lane) & 1ull))) {
                    const unsigned long long rest = lane == 63 ? 0ull : (m.H >> (lane + 1));
                    const int len = rest ? __ffsll(rest) : 64 - lane;
                    const unsigned long long run = (kept >> lane) & (len >= 64 ? ~0ull : ((1ull << len) - 1ull));
                    const unsigned long long bits = run << m.li;
                    it->mlo[m.kk] |= (unsigned)bits;
                    it->mhi[m.kk] |= (unsigned)(bits >> 32);
                }
            }
            gs2m_wave_sync();
            if (rc.staged && rc.tested)   // an untested rect keeps every tile: the scatter does not read a mask for it
                tilemask[(size_t)v * P + gi] = (unsigned long long)it->mlo[k] | ((unsigned long long)it->mhi[k] << 32);
        }
        // ---- rects of more than 64 tiles: the whole wave walks one owner at a time, its fields by shuffle ----
        unsigned long long bigs = gs2m_ballot(rc.wave ? 1 : 0);
        while (bigs != 0ull) {
            const int o = __ffsll(bigs) - 1;
            bigs &= bigs - 1ull;
            const unsigned ow = gs2m_shfl(w, o), oa = gs2m_shfl(area, o), oxy = gs2m_shfl(xy0, o);
            const BinWave ww = bin_wave_begin(ow, oxy, BinGeom{gs2m_shfl(pv[v].mx, o), gs2m_shfl(pv[v].my, o), gs2m_shfl(pv[v].ca, o),
                                                               gs2m_shfl(pv[v].cb, o), gs2m_shfl(pv[v].cc, o), gs2m_shfl(thr, o)});
            for (unsigned li = (unsigned)lane; li < oa; li += 64u) {
                int tile;
                if (bin_wave_tile(ww, li, cull, gx, th, tile)) hist_bump(hh, tile);
            }
        }
    }
}

// Tile counting: same Gaussian -> workgroup assignment as k_scatter.  Re-reads the binning part of the GeomRecs written by
// k_project (and the geometry part of the rects it tests), expands every rect into (Gaussian, tile) pairs (count_expand),
// bumps the workgroup-private LDS tile histogram, records the kept tiles of tested rects as bit masks and writes the
// workgroup's histogram row.
template <int NV>
GS2M_KERNEL void __launch_bounds__(1024)
k_count_tiles(GeomRecs recs, int P, const CamUniform* __restrict__ cams, int chunk, int n_wg,
              unsigned* __restrict__ hist, unsigned long long* __restrict__ tilemask, int exact_cull, int interleave, int lane_tiles) {
    GS2M_DYN_LDS(unsigned, lds);
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = gs2m_uniform(tid >> 6);
    const BinGrid bg = bin_prologue<NV>(cams, recs, P, n_wg, tilemask, hist, exact_cull, lane_tiles);   // moves the four pointers to this group of views
    const int gx = bg.gx, th = bg.th, rs = bg.rs, tiles = bg.tiles, cull = bg.cull;
    // workgroup-private tile histogram: one u32 counter per (view, tile)
    const int nthreads = (int)blockDim.x;
    unsigned* lhist = lds;
    WaveStage* stage = bin_stage<NV, WaveStage>(lds, tiles, wave);
    for (int i = tid; i < NV * tiles; i += nthreads) lhist[i] = 0u;
    __syncthreads();
    const int row = bin_row(n_wg);
    // Two-stage prefetch (round 6).  The 16-B binning part of the records (depth + rect) is loaded TWO wave steps ahead; the 32-B
    // geometry part one step ahead and ONLY for the lanes whose rect is tested -- nothing else of the counting step reads it
    // (round 5 streamed 48 B per (view, Gaussian) through this kernel, 32 of them unused for the thin rects that make up
    // 85 % of a small-splat scene).
    const int nw = nthreads >> 6;
    auto fetch_c = [&](int f0, int e0, float4* c) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            c[v] = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (f0 >= 0 && f0 + lane < e0) c[v] = recs.c[(size_t)v * P + f0 + lane];
        }
    };
    auto fetch_ab = [&](int f0, int e0, const float4* c, float4* a0, float4* a1) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            a0[v] = a1[v] = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (cull && f0 >= 0 && f0 + lane < e0) {
                const BinRect q = bin_rect_of(c[v], rs);
                if (gs2m_rect_tested(q.w, q.h, q.area, cull)) {
                    const size_t ri = (size_t)v * P + f0 + lane;
                    a0[v] = recs.ab[2 * ri];
                    a1[v] = recs.ab[2 * ri + 1];
                }
            }
        }
    };
    float4 c_cur[NV], a0_cur[NV], a1_cur[NV], c_nxt[NV], a0_nxt[NV], a1_nxt[NV], c_nn[NV];
    int end = 0, end_n = 0, end_nn = 0;
    int first = bin_step_begin(0, wave, nw, row, n_wg, chunk, P, interleave, &end);
    int first_n = bin_step_begin(1, wave, nw, row, n_wg, chunk, P, interleave, &end_n);
    fetch_c(first, end, c_cur);
    fetch_c(first_n, end_n, c_nxt);
    fetch_ab(first, end, c_cur, a0_cur, a1_cur);
    for (int it = 0;; ++it) {
        if (first < 0) break;   // wave-uniform; the loop body only uses wave collectives
        const int gi = first + lane;
        const bool valid = gi < end;
        const int first_nn = bin_step_begin(it + 2, wave, nw, row, n_wg, chunk, P, interleave, &end_nn);
        fetch_c(first_nn, end_nn, c_nn);                        // step it + 2: rects
        fetch_ab(first_n, end_n, c_nxt, a0_nxt, a1_nxt);        // step it + 1: geometry where its rect (loaded a step ago) asks for it
        CountIn pv[NV];
        float op = 0.0f;
        bool any_tested = false;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const BinRect q = bin_rect_of(c_cur[v], rs);
            pv[v].ok = valid && q.area != 0u;
            pv[v].x0 = pv[v].ok ? q.x0 : 0;
            pv[v].y0 = pv[v].ok ? q.y0 : 0;
            pv[v].x1 = pv[v].ok ? q.x0 + (int)q.w : 0;
            pv[v].y1 = pv[v].ok ? q.y0 + (int)q.h : 0;
            pv[v].mx = pv[v].my = pv[v].ca = pv[v].cb = pv[v].cc = 0.0f;
            if (pv[v].ok && gs2m_rect_tested(q.w, q.h, q.area, cull)) {
                pv[v].mx = a0_cur[v].x;
                pv[v].my = a0_cur[v].y;
                pv[v].ca = a0_cur[v].z;
                pv[v].cb = a0_cur[v].w;
                pv[v].cc = a1_cur[v].x;
                op = a1_cur[v].y;          // one opacity per Gaussian, whichever view delivered it
                any_tested = true;
            }
        }
        const float thr = any_tested ? cull_threshold(op) : 0.0f;   // one logarithm per tested Gaussian (it was one per view and record)
        count_expand<NV>(pv, thr, valid, gi, P, lhist, tiles, stage, tilemask, gx, th, cull, lane, bg.lane_max);
        first = first_n;
        end = end_n;
        first_n = first_nn;
        end_n = end_nn;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            c_cur[v] = c_nxt[v];
            a0_cur[v] = a0_nxt[v];
            a1_cur[v] = a1_nxt[v];
            c_nxt[v] = c_nn[v];
        }
    }
    __syncthreads();
    for (int v = 0; v < NV; ++v)
        for (int t = tid; t < tiles; t += nthreads) hist[((size_t)v * n_wg + row) * tiles + t] = lhist[v * tiles + t];
}

// Stage of a scatter wave: the item space and the two halves of every owner's sort key (indexed by owner rank k).
struct ScatterStage {
    unsigned dbits[64], gid[64];
    BinItems items;
};

// Instance scatter: same Gaussian -> workgroup assignment as k_count_tiles; cursors start at
// tile_start[v][t] + (exclusive prefix over workgroups, left in `hist` by k_hist_colscan).
// Key = depth_bits << 32 | gaussian_id (unique => order after the per-tile sort is deterministic
// although LDS-atomic arrival order is not).  The walk is the counting pass's (raster_bin_walk.h); tested rects replay the tile
// mask written there, rects of more than 64 tiles repeat the same per-tile test.
template <int NV>
GS2M_KERNEL void __launch_bounds__(1024)
k_scatter(GeomRecs recs, int P, const CamUniform* __restrict__ cams, int chunk, int n_wg,
          const unsigned* __restrict__ hist, const unsigned* __restrict__ tile_start,
          const unsigned long long* __restrict__ tilemask, unsigned long long* __restrict__ keys, unsigned cap,
          int exact_cull, const int* __restrict__ ids, int interleave, int lane_tiles) {
    GS2M_DYN_LDS(unsigned, cursor);
    const int tid = (int)threadIdx.x;
    const int nthreads = (int)blockDim.x;
    const int lane = tid & 63, wave = gs2m_uniform(tid >> 6);
    const BinGrid bg = bin_prologue<NV>(cams, recs, P, n_wg, tilemask, hist, exact_cull, lane_tiles);   // moves the four pointers to this group of views
    const int gx = bg.gx, th = bg.th, rs = bg.rs, tiles = bg.tiles, cull = bg.cull;
    tile_start += (size_t)NV * blockIdx.y * (tiles + 1);
    keys += (size_t)NV * blockIdx.y * cap;
    const int row = bin_row(n_wg);
    for (int v = 0; v < NV; ++v)
        for (int t = tid; t < tiles; t += nthreads)
            cursor[v * tiles + t] = tile_start[(size_t)v * (tiles + 1) + t] + hist[((size_t)v * n_wg + row) * tiles + t];
    __syncthreads();
    const int nw = nthreads >> 6;
    ScatterStage* const stage = bin_stage<NV, ScatterStage>(cursor, tiles, wave);
    BinItems* const it = &stage->items;
    // one view after the other: the key lines this XCD is filling at any time belong to ONE view's array (half the L2
    // working set of a walk that alternates between the views)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        // next-step prefetch (rect + depth vector, id, tile mask) as in k_count_tiles.  (Round 6 measured the counting kernel's
        // two-stage form here -- the mask one step ahead and only for the lanes that replay one: C3 39.8 -> 48 us per pair; this
        // kernel is issue-bound and the second rect decode + the longer rotation cost more than the 8 of 28 bytes saved.)
        float4 n_w2;
        unsigned n_kid;
        unsigned long long n_msk;
        int end = 0;
        int first = bin_step_begin(0, wave, nw, row, n_wg, chunk, P, interleave, &end);
        auto fetch = [&](int f0, int e0) __attribute__((always_inline)) {
            n_w2 = float4{0.0f, 0.0f, 0.0f, 0.0f};
            n_kid = (unsigned)(f0 + lane);
            n_msk = ~0ull;                                       // an untested rect keeps every tile
            if (f0 >= 0 && f0 + lane < e0) {
                if (ids) n_kid = (unsigned)ids[f0 + lane];
                n_w2 = recs.c[(size_t)v * P + f0 + lane];   // the 16-B binning part only: contiguous, fully used lines
                if (cull) n_msk = tilemask[(size_t)v * P + f0 + lane];   // only meaningful (and only used) for tested rects of <= 64 tiles
            }
        };
        fetch(first, end);
        for (int step = 0;; ++step) {
            if (first < 0) break;   // wave-uniform
            const int gi = first + lane;
            const bool valid = gi < end;
            const float4 w2 = n_w2;
            const unsigned kid = n_kid;   // low word of the sort key: the Gaussian's id (ties in depth resolve as in the reference)
            unsigned long long msk_pre = n_msk;
            {
                int end_next = 0;
                const int first_next = bin_step_begin(step + 1, wave, nw, row, n_wg, chunk, P, interleave, &end_next);
                fetch(first_next, end_next);
                first = first_next;      // rotated here: the wave-uniform `continue` below skips nothing of the pipeline
                end = end_next;
            }
            const BinRect q = bin_rect_of(w2, rs);
            const unsigned dbits = __float_as_uint(w2.y);
            const unsigned xy0 = (unsigned)q.x0 | ((unsigned)q.y0 << 16);
            const unsigned w = q.w, h = q.h, area = valid ? q.area : 0u;
            if (gs2m_ballot(area != 0u ? 1 : 0) == 0ull) continue;  // wave-uniform
            const BinClass rc = bin_rect_class(w, h, area, cull, bg.lane_max, false);
            if (!rc.tested) msk_pre = ~0ull;   // the word loaded for an untested rect is not a mask
            unsigned* cur = cursor + v * tiles;
            unsigned long long* kv = keys + (size_t)v * cap;
            // rects walked by their own lane: the lane emits its own keys, replaying its mask (all ones when the rect was not
            // tested), row-major bits
            if (gs2m_ballot(rc.lane ? 1 : 0) != 0ull) {
                const unsigned area_l = rc.lane ? area : 0u;
                const unsigned long long key = ((unsigned long long)dbits << 32) | kid;
                BinLaneCursor c = bin_lane_begin(q.x0, q.y0, gx);
                // four tiles per round: the (returning) LDS atomics of a round are issued back to back and waited for ONCE, then
                // the key stores (rounds 4-5 ran one atomic -> wait -> store chain per tile: four LDS round trips in sequence
                // for a 2 x 2 rect)
                for (unsigned t0 = 0; t0 < area_l; t0 += 4u) {
                    unsigned pos[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const unsigned t = t0 + (unsigned)u;
                        pos[u] = cap;
                        if (t < area_l && ((msk_pre >> t) & 1ull) != 0ull) pos[u] = atomicAdd(&cur[c.tile], 1u);
                        bin_lane_next(c, w, gx);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (pos[u] < cap) kv[pos[u]] = key;
                }
            }
            const unsigned long long stageds = gs2m_ballot(rc.staged ? 1 : 0);
            if (stageds != 0ull) {
                int k;
                const unsigned total = bin_items_build(it, lane, rc.staged, stageds, w, h, area, xy0, rc.tested, msk_pre, k,
                                                       [&](int ko) __attribute__((always_inline)) {
                    stage->dbits[ko] = dbits;
                    stage->gid[ko] = kid;
                });
                int kbase = 0;
                // one 64-item batch: owner lookup, mask bit, cursor bump -> (position, key) of this lane's item (position `cap`: none)
                auto emit = [&](unsigned b0, unsigned& pos, unsigned long long& key) __attribute__((always_inline)) {
                    pos = cap;
                    key = 0ull;
                    bin_item(it, b0, total, lane, kbase, [&](const BinItem& m) __attribute__((always_inline)) {
                        const unsigned long long om = (unsigned long long)it->mlo[m.kk] | ((unsigned long long)it->mhi[m.kk] << 32);
                        const bool keep = ((om >> m.li) & 1ull) != 0ull;
                        if (keep) {
                            int tx, ty;
                            bin_item_tile(it, m, tx, ty);
                            key = ((unsigned long long)stage->dbits[m.kk] << 32) | stage->gid[m.kk];
                            pos = atomicAdd(&cur[ty * gx + tx], 1u);
                        }
                        return keep;
                    });
                };
                // two batches per round, the key store of a batch BEHIND the next batch's cursor bump: the returning LDS atomic of
                // batch A is waited for together with the stage reads of batch B (LDS operations return in order), not on its own
                // (rounds 1-5: reads -> wait -> atomic -> wait -> store, per batch)
                unsigned pos_a, pos_b = cap;
                unsigned long long key_a, key_b = 0ull;
                for (unsigned b0 = 0; b0 < total; b0 += 128u) {
                    emit(b0, pos_a, key_a);
                    if (pos_b < cap) kv[pos_b] = key_b;
                    pos_b = cap;
                    if (b0 + 64u < total) emit(b0 + 64u, pos_b, key_b);
                    if (pos_a < cap) kv[pos_a] = key_a;
                }
                if (pos_b < cap) kv[pos_b] = key_b;
            }
            // rects of more than 64 tiles (rare): the whole wave walks one owner at a time, its geometry from the record
            unsigned long long bigs = gs2m_ballot(rc.wave ? 1 : 0);
            while (bigs != 0ull) {
                const int o = __ffsll(bigs) - 1;
                bigs &= bigs - 1ull;
                const unsigned ow = gs2m_shfl(w, o), oa = gs2m_shfl(area, o), oxy = gs2m_shfl(xy0, o);
                const unsigned long long key = ((unsigned long long)gs2m_shfl(dbits, o) << 32) | gs2m_shfl(kid, o);
                BinGeom og{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (cull) {
                    const float4* r4 = recs.ab + 2 * ((size_t)v * P + gs2m_shfl(gi, o));
                    const float4 w0 = r4[0];
                    const float4 w1 = r4[1];
                    og = BinGeom{w0.x, w0.y, w0.z, w0.w, w1.x, cull_threshold(w1.y)};
                }
                const BinWave ww = bin_wave_begin(ow, oxy, og);
                for (unsigned li = (unsigned)lane; li < oa; li += 64u) {
                    int tile;
                    if (bin_wave_tile(ww, li, cull, gx, th, tile)) {
                        const unsigned pos = atomicAdd(&cur[tile], 1u);
                        if (pos < cap) kv[pos] = key;
                    }
                }
            }
        }
    }
}

// One-time re-layout of the SH block for the pipeline-level path (Renderer.prepare_renderer): the
// reference layout is one 192-B row per Gaussian ([P,16,3], or dc [P,1,3] + rest [P,15,3]), which a
// thread-per-Gaussian kernel reads as 12 float4 loads strided by 192 B (64 cache lines per wave
// instruction, L1 thrash).  Packed: [P/64][12][64] float4 -- every load instruction of a wave is one
// contiguous KiB.
// `order` (null = identity): position gi of the packed copy holds Gaussian order[gi] (gs2m_raster_pack_model).
GS2M_KERNEL void __launch_bounds__(256)
k_pack_sh(int P, const float* __restrict__ shs, const float* __restrict__ shs_rest, float* __restrict__ packed,
          const int* __restrict__ order) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // one float of the [P,48] matrix
    if (i >= (size_t)P * 48) return;
    const size_t gi = i / 48;
    const int c = (int)(i - gi * 48);
    const size_t src = order ? (size_t)order[gi] : gi;
    float v;
    if (shs_rest == nullptr) v = shs[src * 48 + c];
    else v = c < 3 ? shs[src * 3 + c] : shs_rest[src * 45 + (c - 3)];
    const int k = c >> 2, e = c & 3;
    packed[(((gi >> 6) * 12 + k) * 64 + (gi & 63)) * 4 + e] = v;
}

// Spatially ordered packed copy of the per-Gaussian parameters (gs2m_raster_pack_model): position j <- Gaussian
// order[j]; rank[order[j]] = j is the inverse the compositing stage uses to find a record from the id in a sort key.
GS2M_KERNEL void __launch_bounds__(256)
k_pack_model(int P, const int* __restrict__ order, const float* __restrict__ xyz, const float* __restrict__ scales,
             const float* __restrict__ rots, const float* __restrict__ opac, float* __restrict__ p_xyz,
             float* __restrict__ p_scales, float* __restrict__ p_rots, float* __restrict__ p_opac, int* __restrict__ rank) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= P) return;
    const int id = order[j];
    if (id < 0 || id >= P) return;   // not a permutation: rank keeps a hole, k_check_rank reports it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p_xyz[3 * (size_t)j + c] = xyz[3 * (size_t)id + c];
        p_scales[3 * (size_t)j + c] = scales[3 * (size_t)id + c];
    }
    *reinterpret_cast<float4*>(p_rots + 4 * (size_t)j) = *reinterpret_cast<const float4*>(rots + 4 * (size_t)id);
    p_opac[j] = opac[id];
    rank[id] = j;
}

// order is a permutation of 0..P-1 <=> every rank entry was written exactly once (holes stay -1)
GS2M_KERNEL void __launch_bounds__(256)
k_check_rank(int P, const int* __restrict__ rank, const int* __restrict__ order, unsigned* __restrict__ bad) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    const int j = rank[i];
    if (j < 0 || j >= P || order[j] != i) atomicOr(bad, 1u);
}

// checkFrustum (rasterizer_impl.cu:54-66): present = z_view > 0.2
GS2M_KERNEL void __launch_bounds__(256)
k_mark_visible(int P, const float* __restrict__ xyz, const float* __restrict__ viewmatrix,
               unsigned char* __restrict__ present) {
    const int gi = (int)(blockIdx.x * 256u + threadIdx.x);
    if (gi < P) {
        float tx, ty, tz;
        xform4x3(viewmatrix, xyz[3 * (size_t)gi], xyz[3 * (size_t)gi + 1], xyz[3 * (size_t)gi + 2], tx, ty, tz);
        present[gi] = tz <= 0.2f ? 0 : 1;
    }
}

// Fill the device CamUniform of view `slot` from DEVICE pointers (operator-level API, where
// viewmatrix / projmatrix / campos / bg are device tensors as in the reference).
GS2M_KERNEL void k_pack_camera(CamUniform* cams, int slot, const float* viewmatrix, const float* projmatrix,
                               const float* campos, const float* bg, float tanfovx, float tanfovy, int W, int H,
                               int th) {
    const int t = (int)threadIdx.x;
    CamUniform* c = cams + slot;
    if (t < 16) {
        c->view[t] = viewmatrix[t];
        c->proj[t] = projmatrix[t];
    }
    if (t < 3) {
        c->campos[t] = campos[t];
        c->bg[t] = bg[t];
    }
    if (t == 0) {
        c->tanfovx = tanfovx;
        c->tanfovy = tanfovy;
        c->focal_y = H / (2.0f * tanfovy);  // rasterizer_impl.cu:222-223
        c->focal_x = W / (2.0f * tanfovx);
        c->W = W;
        c->H = H;
        c->gx = (W + GS2M_TILE - 1) / GS2M_TILE;
        c->gy = (H + GS2M_TILE - 1) / GS2M_TILE;
        c->th = th;
    }
}
