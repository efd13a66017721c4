// raster_internal.h -- launch wrappers shared between the translation units of the rasteriser.
// Each .hip file is compiled on its own so that per-stage floating-point contraction can
// differ (projection: -ffp-contract=off for a literal IEEE sequence; blend: default fast
// contraction, FMA).
#pragma once
#include "api_check.h"
#include "raster_common.h"

size_t gs2m_scatter_lds_bytes(int nv, int tiles, int threads);
// host_cams: null (the uniforms are already in `cams`, device memory) or the nv * pairs host-side uniforms of the pass (carried in
// the launch packet; the kernel also stores them to `cams`)
void gs2m_launch_project(int nv, int pairs, hipStream_t st, const GaussIn& g, CamUniform* cams, GeomRecs recs, int* radii,
                         int exact_cull, const CamUniform* host_cams, int shared_read);
int gs2m_launch_count_tiles(int nv, int pairs, int n_wg, int threads, size_t lds_bytes, hipStream_t st, GeomRecs recs, int P,
                            const CamUniform* cams, int chunk, unsigned* hist, unsigned long long* tilemask,
                            int exact_cull, int interleave, int lane_tiles);
int gs2m_count_threads(int chunk, int max_threads);
size_t gs2m_count_lds_bytes(int nv, int tiles, int threads);
int gs2m_launch_scatter(int nv, int pairs, int n_wg, int threads, size_t lds_bytes, hipStream_t st, GeomRecs recs, int P,
                        const CamUniform* cams, int chunk, const unsigned* hist, const unsigned* tile_start,
                        const unsigned long long* tilemask, unsigned long long* keys, unsigned cap, int exact_cull,
                        const int* ids, int interleave, int lane_tiles);
void gs2m_launch_pack_sh(hipStream_t st, int P, const float* shs, const float* shs_rest, float* packed, const int* order);
void gs2m_launch_pack_model(hipStream_t st, int P, const int* order, const float* xyz, const float* scales, const float* rots,
                            const float* opac, float* p_xyz, float* p_scales, float* p_rots, float* p_opac, int* rank,
                            unsigned* bad);
void gs2m_launch_mark_visible(hipStream_t st, int P, const float* xyz, const float* viewmatrix,
                              unsigned char* present);
void gs2m_launch_pack_camera(hipStream_t st, CamUniform* cams, int slot, const float* viewmatrix,
                             const float* projmatrix, const float* campos, const float* bg, float tanfovx,
                             float tanfovy, int W, int H, int th);

void gs2m_launch_hist_colscan(hipStream_t st, int nv, unsigned* hist, int n_wg, int tiles, unsigned* tile_count);
void gs2m_launch_tile_scan(hipStream_t st, int nv, const unsigned* tile_count, unsigned* tile_start, int tiles, int gx,
                           ViewStatus* status, ViewStatus* sticky, unsigned cap, unsigned* sort_lists);
size_t gs2m_sort_lists_words(int nv, int tiles);
void gs2m_launch_sort_tiles(hipStream_t st, int nv, unsigned long long* keys, unsigned long long* tmp,
                            const unsigned* tile_start, int tiles, unsigned cap, const unsigned* sort_lists, const int* class_hint);
int gs2m_launch_blend(hipStream_t st, int variant, int tile_rows, int nv, int gx, int gy, const unsigned long long* keys,
                      const unsigned* tile_start, GeomRecs recs, const CamUniform* cams, int P,
                      unsigned cap, float* out_color, unsigned char* out_rgb8, const int* rank, const unsigned* order,
                      int mode, unsigned long long* prof, int interleave_views);

// ---- backward pass (gs2m_rasterize_backward): outputs of the per-Gaussian kernel, device pointers
struct BwOut {
    float* dL_dmean2D;   // [P,3]
    float* dL_dconic;    // null or [P,4]: {a, b, 0, c} (the reference's [P,2,2] tap)
    float* dL_dopacity;  // [P]
    float* dL_dcolor;    // [P,3]
    float* dL_dmean3D;   // [P,3]
    float* dL_dcov3D;    // [P,6]
    float* dL_dsh;       // null or [P,M,3]
    float* dL_dscale;    // [P,3]
    float* dL_drot;      // [P,4]
};
// exclusive scan of the records' tile-rect areas -> row_offset[P] (first instance row of every Gaussian), *total_rows = their sum;
// block_sum = scratch of ceil(P / 256) words
void gs2m_launch_bw_row_offsets(hipStream_t st, GeomRecs recs, int P, unsigned* block_sum, unsigned* row_offset,
                                unsigned long long* total_rows);
// depth = 0: the colour backward (dL_dpix required, the three map gradients not read, row value 9 neither written nor read);
// depth = 1: the instantiations with the depth / opacity map terms (gs2m_rasterize_backward_depth): dL_dpix and each of
// dL_ddepth / dL_dmedian / dL_dalpha ([H,W]) may be null = zeros.  Both launches of one backward take the same flag.
void gs2m_launch_blend_backward(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                GeomRecs recs, const CamUniform* cams, int P, unsigned cap, const float* dL_dpix,
                                const unsigned* row_offset, float* rows, unsigned long long n_rows, int depth,
                                const float* dL_ddepth, const float* dL_dmedian, const float* dL_dalpha);
void gs2m_launch_gaussian_backward(hipStream_t st, const GaussIn& g, const CamUniform* cams, GeomRecs recs,
                                   const unsigned* row_offset, const float* rows, unsigned long long n_rows, const BwOut& out,
                                   int depth);
// ---- gradients through the ray maps (gs2m_rasterize_backward_depth_ray).  The compositing half is the depth instantiation with
// z_j(p) of the ray records and a second row of GS2M_BW_ROW floats per instance in rows2 (raster_backward_blend.h); the
// per-Gaussian half runs AFTER gs2m_launch_gaussian_backward(depth = 1) and adds to dL_dmean3D, dL_dscale and dL_drot.
void gs2m_launch_blend_backward_ray(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                    GeomRecs recs, const CamUniform* cams, int P, unsigned cap, const float* dL_dpix,
                                    const unsigned* row_offset, float* rows, float* rows2, unsigned long long n_rows,
                                    const float4* ray, const float* dL_ddepth, const float* dL_dmedian, const float* dL_dalpha);
void gs2m_launch_gaussian_backward_ray(hipStream_t st, const GaussIn& g, const CamUniform* cams, GeomRecs recs,
                                       const unsigned* row_offset, const float* rows2, unsigned long long n_rows,
                                       const BwOut& out);

// ---- depth / opacity maps (gs2m_rasterize_depth): [H,W] f32 each, any of them null
void gs2m_launch_blend_depth(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                             GeomRecs recs, int P, unsigned cap, int W, int H, float* depth_expected, float* depth_median,
                             float* alpha);
// ---- ray-Gaussian intersection depth (gs2m_rasterize_depth_ray): ray[P][4] float4, written for the Gaussians with a tile rect
void gs2m_launch_ray_records(hipStream_t st, GeomRecs recs, int P, const float* means3D, const float* scales, float scale_modifier,
                             const float* rotations, const float* viewmatrix, float4* ray);
void gs2m_launch_blend_depth_ray(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                 GeomRecs recs, int P, unsigned cap, int W, int H, const float4* ray, float tanfovx,
                                 float tanfovy, float* depth_expected, float* depth_median, float* alpha);
