// raster_blend.hip -- compositing stage (default FMA contraction; VALU-bound inner loop).
#include "raster_blend.h"
#include "raster_backward_blend.h"
#include "raster_depth.h"
#include "raster_internal.h"

// gy = rows of the 16 x 16 reference grid; tile_rows = 16 x 16 tiles per instance list (GS2M_OPT_TILE_ROWS)
//   variant 4: wave-per-tile kernel (k_blend_wave4e),
//   0: the reference's structure (256-thread workgroup per tile, 1 pixel per lane; 16 x 16 lists only)
int gs2m_launch_blend(hipStream_t st, int variant, int tile_rows, int nv, int gx, int gy, const unsigned long long* keys,
                      const unsigned* tile_start, GeomRecs recs, const CamUniform* cams, int P, unsigned cap,
                      float* out_color, unsigned char* out_rgb8, const int* rank, const unsigned* order, int mode,
                      unsigned long long* prof, int interleave_views) {
    const dim3 block(256);
    if (variant == 4) {
        const int ltiles = gx * ((gy + tile_rows - 1) / tile_rows);
        // schedule: ceil(chunks / 8) chunks per XCD, GS2M_SCHED_CHUNK lists per chunk, tile_rows waves per list, 4 waves per workgroup
        const int nch = ((gx + GS2M_SCHED_CW - 1) / GS2M_SCHED_CW) * ((ltiles / gx + GS2M_SCHED_CH - 1) / GS2M_SCHED_CH);
        const dim3 g2(8u * ((unsigned)(((nch + 7) / 8) * GS2M_SCHED_CHUNK * tile_rows + 3) / 4u), nv);
        if (mode >= 2) {   // GS2M_OPT_BLEND_MODE 2 / 3 (round 5): all four quadrants per instance, flag-free runs; views interleaved along x
            // interleaved: one row of blocks, view = (blockIdx.x / 8) % nv; else the views along blockIdx.y
            const int nvx = interleave_views && nv > 1 ? nv : 0;
            const dim3 g1 = nvx ? dim3(g2.x * (unsigned)nv, 1) : g2;
            if (prof) {   // GS2M_OPT_BLEND_PROFILE: the same kernel with s_memtime phase stamps
                if (tile_rows == 2) GS2M_LAUNCH((k_blend_wave4e<4, 2, 7, 2, 1>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, prof, nvx);
                else GS2M_LAUNCH((k_blend_wave4e<4, 1, 7, 2, 1>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, prof, nvx);
                return 0;
            }
            if (mode == 3) {   // mode 2 with the alpha cap for every instance (no run split at capped instances)
                if (tile_rows == 2) GS2M_LAUNCH((k_blend_wave4e<4, 2, 7, 3>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr, nvx);
                else GS2M_LAUNCH((k_blend_wave4e<4, 1, 7, 3>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr, nvx);
                return 0;
            }
            if (tile_rows == 2) GS2M_LAUNCH((k_blend_wave4e<4, 2, 7, 2>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr, nvx);
            else GS2M_LAUNCH((k_blend_wave4e<4, 1, 7, 2>), g1, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr, nvx);
            return 0;
        }
        // GS2M_OPT_BLEND_MODE 0: the lane-mask loop of rounds 1-4 (cross-check of mode 2)
        if (tile_rows == 2) GS2M_LAUNCH((k_blend_wave4e<4, 2, 7>), g2, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr);
        else GS2M_LAUNCH((k_blend_wave4e<4, 1, 7>), g2, block, 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank, order, nullptr);
        return 0;
    }
    if (variant == 0 && tile_rows == 1) {
        GS2M_LAUNCH(k_blend_tile256, dim3(gx, gy, nv), dim3(256), 0, st, keys, tile_start, recs, cams, P, cap, out_color, out_rgb8, rank);
        return 0;
    }
    gs2m_set_error("blend variant %d is not available with GS2M_OPT_TILE_ROWS %d (variants: 0 [rows 1 only], 4)", variant, tile_rows);
    return 1;
}

// backward of the compositing (one view, 16 x 16 lists): one wave per tile, four tiles per workgroup
void gs2m_launch_blend_backward(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                GeomRecs recs, const CamUniform* cams, int P, unsigned cap, const float* dL_dpix,
                                const unsigned* row_offset, float* rows, unsigned long long n_rows, int depth,
                                const float* dL_ddepth, const float* dL_dmedian, const float* dL_dalpha) {
    const int tiles = gx * gy;
    const BwDepthGrads dg{dL_ddepth, dL_dmedian, dL_dalpha};
    if (depth)
        GS2M_LAUNCH((k_blend_backward<4, true>), dim3((tiles + 3) / 4), dim3(256), 0, st, keys, tile_start, recs, cams, P, cap,
                    dL_dpix, row_offset, rows, n_rows, dg);
    else
        GS2M_LAUNCH((k_blend_backward<4, false>), dim3((tiles + 3) / 4), dim3(256), 0, st, keys, tile_start, recs, cams, P, cap,
                    dL_dpix, row_offset, rows, n_rows, dg);
}

// the depth instantiation with the ray-Gaussian intersection depth (gs2m_rasterize_backward_depth_ray): `ray` = the records of
// gs2m_launch_ray_records, rows2 = the second row of every instance (cleared like `rows`)
void gs2m_launch_blend_backward_ray(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                    GeomRecs recs, const CamUniform* cams, int P, unsigned cap, const float* dL_dpix,
                                    const unsigned* row_offset, float* rows, float* rows2, unsigned long long n_rows,
                                    const float4* ray, const float* dL_ddepth, const float* dL_dmedian, const float* dL_dalpha) {
    const int tiles = gx * gy;
    const BwDepthGrads dg{dL_ddepth, dL_dmedian, dL_dalpha};
    GS2M_LAUNCH((k_blend_backward<4, true, true>), dim3((tiles + 3) / 4), dim3(256), 0, st, keys, tile_start, recs, cams, P, cap,
                dL_dpix, row_offset, rows, n_rows, dg, ray, rows2);
}

// depth / opacity maps of the last single-view forward (16 x 16 lists): one wave per tile, four tiles per workgroup
void gs2m_launch_blend_depth(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                             GeomRecs recs, int P, unsigned cap, int W, int H, float* depth_expected, float* depth_median,
                             float* alpha) {
    const int tiles = gx * gy;
    GS2M_LAUNCH((k_blend_depth<4>), dim3((tiles + 3) / 4), dim3(256), 0, st, keys, tile_start, recs, P, cap, W, H, gx, gy,
                depth_expected, depth_median, alpha, (const float4*)nullptr, 0.0f, 0.0f);
}

// ray records of the Gaussians the last forward listed (raster_depth_ray.h): one lane per Gaussian
void gs2m_launch_ray_records(hipStream_t st, GeomRecs recs, int P, const float* means3D, const float* scales, float scale_modifier,
                             const float* rotations, const float* viewmatrix, float4* ray) {
    GS2M_LAUNCH(k_ray_records, dim3((P + 255) / 256), dim3(256), 0, st, recs, P, means3D, scales, scale_modifier, rotations,
                viewmatrix, ray);
}

// the walk of gs2m_launch_blend_depth with the ray-Gaussian intersection depth of every (instance, pixel)
void gs2m_launch_blend_depth_ray(hipStream_t st, int gx, int gy, const unsigned long long* keys, const unsigned* tile_start,
                                 GeomRecs recs, int P, unsigned cap, int W, int H, const float4* ray, float tanfovx,
                                 float tanfovy, float* depth_expected, float* depth_median, float* alpha) {
    const int tiles = gx * gy;
    GS2M_LAUNCH((k_blend_depth<4, true>), dim3((tiles + 3) / 4), dim3(256), 0, st, keys, tile_start, recs, P, cap, W, H, gx, gy,
                depth_expected, depth_median, alpha, ray, tanfovx, tanfovy);
}
