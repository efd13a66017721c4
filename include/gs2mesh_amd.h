/*
 * gs2mesh_amd.h -- C ABI of the MI355X-native render -> fuse hot path of GS2Mesh.
 *
 * This is the drop-in boundary: a plain C shared library (libgs2mesh_amd.so, HIP/gfx950)
 * with raw device pointers, sizes and a hipStream_t.  No torch types cross it.  The
 * Python host side (package gs2mesh_amd) binds it with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Citations are file:line in the reference tree (/root/reference), with
 *   DGR/ = third_party/gaussian-splatting/submodules/diff-gaussian-rasterization/
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; gs2m_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - all `const float*` / `float*` / `uint8_t*` data arguments are DEVICE pointers
 *     unless the comment says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued on it, nothing synchronises the device except the functions that say
 *     so (gs2m_raster_status, gs2m_tsdf_status, the *_download helpers);
 *   - handles own persistent, grow-only scratch arenas (the reference re-allocates
 *     its three byte arenas every call: DGR/rasterize_points.cu:27-33,73-78).  A
 *     handle may only be used from one stream at a time.
 */
#ifndef GS2MESH_AMD_H
#define GS2MESH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_VERSION 600 /* 0.6.0: round-6 ABI = the round-4 ABI (401) + the round-5 entry points that 401 never counted
                            (gs2m_tsdf_block_map / _map_keys / _map_bytes / _replace / _extract_mesh / _mesh_copy,
                            gs2m_mesh_cluster, gs2m_raster_blend_cycles, GS2M_OPT_BLEND_MODE / _PROFILE) + round 6
                            (gs2m_tsdf_flags_device, GS2M_OPT_BIN_LANE_TILES, GS2M_OPT_PROJECT_SHARED_READ, GS2M_OPT_EXACT_TILE_CULL level 2; GS2M_OPT_BLEND_MODE 1
                            removed).  Added since without a new number: gs2m_stereo_sgm / gs2m_stereo_sgm_scratch_bytes,
                            gs2m_knn_mean_dist2 / gs2m_knn_scratch_bytes, gs2m_photo_loss_forward / _backward /
                            _scratch_bytes, gs2m_adam_step, gs2m_densify_stats, gs2m_icp_prepare / _step / _scratch_bytes,
                            gs2m_voxel_mean, gs2m_depth_consistency.  The Python binding checks it at load time */

typedef void* gs2m_stream; /* hipStream_t */

/* ------------------------------------------------------------------------------------ */
/* library                                                                              */
/* ------------------------------------------------------------------------------------ */

int gs2m_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* gs2m_last_error(void);

/* ------------------------------------------------------------------------------------ */
/* rasteriser                                                                           */
/* ------------------------------------------------------------------------------------ */

typedef struct gs2m_raster gs2m_raster;

/* Flags for gs2m_raster_set_option */
enum {
    GS2M_OPT_EXACT_TILE_CULL = 1, /* 0 = reference AABB-of-3-sigma-circle instance list
                                     (DGR/cuda_rasterizer/auxiliary.h:46-56), 1 = also drop
                                     (Gaussian,tile) instances whose alpha < 1/255 on the
                                     whole tile (image unchanged, num_rendered smaller);
                                     2 (round 6) = the same, but rects of at most 4 binning tiles
                                     keep all their tiles (the per-tile test removes ~2 % of the
                                     instances of a small-splat scene and was 60 % of the vector
                                     instructions of the counting kernel)                 */
    GS2M_OPT_BLEND_VARIANT = 2,   /* compositing kernel: 4 (default) = one wave per 16x16 tile, 4 pixels per lane;
                                     0 = the reference's structure (16x16 tile per 256-thread workgroup,
                                     1 px/lane; GS2M_OPT_TILE_ROWS 1 only).  Same image (to rounding).
                                     (7, exponents on the matrix cores, was removed in round 3: slower than 4
                                     and wrong on strongly anisotropic splats -- DESIGN.md 3.) */
    GS2M_OPT_DEBUG_SYNC = 3,      /* 1 = synchronise + check after every launch (the
                                     reference's `debug`: auxiliary.h:166-173)            */
    GS2M_OPT_STAGE_TIMING = 4,    /* 1 = bracket every stage launch with hipEvents on the
                                     work stream (read with gs2m_raster_stage_times)      */
    GS2M_OPT_PAIR_BATCH = 8,      /* gs2m_render_views: up to `value` (2 .. 4; 0 / 1 = off, the default) stereo pairs share every launch
                                     of a pass, as far as the call has them (the projection / counting / scatter workgroups of a pair are
                                     1 / pairs as many, blockIdx.y picks the pair; scans, per-tile sort and compositing take all the views
                                     in one grid): the per-launch and per-workgroup fixed costs are paid once, and the compositing grid
                                     is long against its tail.  Same results. */
    /* Tuning options (results never change; defaults are the measured optima, profiles/r3_experiments.txt): */
    GS2M_OPT_BIN_WORKGROUPS = 9,  /* workgroups of the counting / scatter kernels per stereo pair (default 0 = 256, one per CU: the
                                     per-workgroup histogram rows / cursors scale with their number) */
    GS2M_OPT_BIN_WG_THREADS = 10, /* upper bound of their threads per workgroup, a multiple of 64 (default 0 = 1024) */
    GS2M_OPT_BLEND_MODE = 11,     /* compositing loop of variant 4 (three forms of the same arithmetic, bit-identical images):
                                     2 (default, round 5) = every staged instance evaluates all four 8x8 quadrants, candidate
                                     test = one v_cmp against the lane's own threshold, accumulate under the execution mask,
                                     the alpha-cap / power > 0 instances split out per run of the staged batch;
                                     3 (round 6) = 2 with min(0.99, alpha) applied to EVERY instance (the identity where the cap
                                     cannot bind) instead of splitting the runs at the instances whose opacity exceeds 0.98: for
                                     models with many saturated opacities (a trained splat: ~30 %; -10 % compositing time there,
                                     +3.6 % on a model with 2 %) -- rasterizer.auto_blend_mode picks by the model's share;
                                     0 = per-pixel decisions as lane masks in scalar registers + per-instance quadrant mask
                                     (the loop of rounds 1-4, kept as the cross-check).  (1, the execution-mask form of 0, was
                                     never the fastest anywhere and was removed in round 6.) */
    GS2M_OPT_BLEND_PROFILE = 12,  /* 1 = launch the s_memtime-instrumented build of the compositing kernel (mode 2 only) and sum
                                     its per-wave phase cycles in the handle; read with gs2m_raster_blend_cycles */
    GS2M_OPT_BIN_LANE_TILES = 13, /* tuning (results never change): a tile rect of at most `value` binning tiles (0 .. 16, default 4) is
                                     walked by its own lane in the counting / scatter kernels -- exact tile test in registers, the kept
                                     tiles as a small bit mask -- instead of through the wave-balanced staged walk; 0 = only the thin
                                     rects of round 4 (one tile wide or high, <= 4 tiles) */
    GS2M_OPT_PROJECT_SHARED_READ = 14, /* tuning (results never change): the stereo pairs of a launch (GS2M_OPT_PAIR_BATCH) share ONE read of
                                     the model in the projection kernel -- the thread that owns a Gaussian projects it for every pair of
                                     the launch -- instead of one grid row per pair.  0 (default) = with a spatially ordered packed model
                                     (gs2m_raster_pack_model) or from 1 000 000 Gaussians (a small unordered model re-reads from the
                                     last-level cache and prefers twice the waves), 1 = always, 2 = never */
    GS2M_OPT_TILE_ROWS = 5        /* binning tile = 16 x (16 * rows) pixels.  1 (default) = the reference's 16 x 16
                                     tiles: instance lists / num_rendered are the reference's.  2 = two reference
                                     tiles stacked: ~30 % fewer (Gaussian, tile) instances to count, scatter and
                                     sort; two waves share a list, each compositing its 16 x 16 half; same image -- the reference's
                                     16 x 16 tile rect still bounds every contribution.  The binning taps then
                                     describe the 16 x 32 tiles.                                            */
};

/* Stage order of gs2m_raster_stage_times */
enum {
    GS2M_STAGE_PROJECT = 0, /* k_project       */
    GS2M_STAGE_COLSCAN = 1, /* k_hist_colscan  */
    GS2M_STAGE_TILESCAN = 2,/* k_tile_scan     */
    GS2M_STAGE_SCATTER = 3, /* k_scatter       */
    GS2M_STAGE_SORT = 4,    /* k_sort_tiles    */
    GS2M_STAGE_BLEND = 5,   /* k_blend_*       */
    GS2M_STAGE_COUNT = 6,   /* k_count_tiles (runs between PROJECT and COLSCAN) */
    GS2M_N_STAGES = 7
};

int gs2m_raster_create(gs2m_raster** out, int device);
int gs2m_raster_destroy(gs2m_raster* r);
int gs2m_raster_set_option(gs2m_raster* r, int option, int value);

/* Pre-size the arenas (optional; every forward grows them on demand).
 * P Gaussians, n_views views of W x H rendered per call, `instances` (Gaussian,tile)
 * pairs per view (the reference's num_rendered). */
int gs2m_raster_reserve(gs2m_raster* r, int P, int n_views, int W, int H, int64_t instances);

/*
 * Operator-level entry point.  Replaces CudaRasterizer::Rasterizer::forward
 * (DGR/cuda_rasterizer/rasterizer.h:35-60, rasterizer_impl.cu:198-336) as bound by
 * RasterizeGaussiansCUDA (DGR/rasterize_points.cu:35-115): same argument meaning and order,
 * minus the three std::function arena callbacks (arenas live in the handle) plus the
 * handle and the stream.
 *
 *   P, D, M           #Gaussians, active SH degree (0..3), #SH coefficients per channel
 *   background[3]     device
 *   means3D[P,3]      device
 *   shs[P,M,3]        device or NULL (then colors_precomp must be given)
 *   colors_precomp[P,3] device or NULL
 *   opacities[P]      device (activated)
 *   scales[P,3], rotations[P,4] (wxyz)  device (activated) or NULL (then cov3D_precomp)
 *   cov3D_precomp[P,6] device or NULL
 *   viewmatrix[16], projmatrix[16], cam_pos[3]   device, the reference's transposed
 *                     row-major layout (GS/scene/cameras.py:54-57)
 *   out_color[3,H,W]  device, written completely
 *   radii[P]          device or NULL
 *   debug             as the reference: sync + check after every launch
 *
 * Asynchronous.  If the instance arena was too small the image is NOT valid; query
 * gs2m_raster_status() (which synchronises the stream), gs2m_raster_reserve() and
 * call again -- the Python binding does exactly that.
 */
int gs2m_rasterize_forward(gs2m_raster* r, int P, int D, int M, const float* background,
                           int width, int height, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities,
                           const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix,
                           const float* projmatrix, const float* cam_pos, float tan_fovx,
                           float tan_fovy, int prefiltered, float* out_color, int* radii,
                           int debug, gs2m_stream stream);

/*
 * Backward pass of the LAST gs2m_rasterize_forward on this handle (3DGS training gradients).  Replaces
 * CudaRasterizer::Rasterizer::backward (rasterizer.h:55-84, rasterizer_impl.cu:338-434): same argument meaning and order,
 * minus `radii` and the three arenas (the projected records, the sorted per-tile lists and the ranges are still in the
 * handle) plus the handle and the stream.  The inputs must be the ones the forward was called with.
 *
 *   R                 num_rendered of the forward (informational: the handle knows it)
 *   dL_dpix[3,H,W]    device, gradient of the loss by the forward's out_color
 *   dL_dmean2D[P,3]   device: NDC-scaled (0.5 W, 0.5 H), z = 0 -- what training's densification reads from means2D.grad
 *   dL_dconic[P,4]    device or NULL: {a, b, 0, c} (the reference's [P,2,2] intermediate; a tap).  As in the reference, b is
 *                     HALF the derivative by conic.y (backward.cu:550; its cov2D formulas expect that)
 *   dL_dopacity[P], dL_dcolor[P,3], dL_dmean3D[P,3], dL_dcov3D[P,6], dL_dscale[P,3], dL_drot[P,4]   device
 *   dL_dsh[P,M,3]     device (required with shs; coefficients beyond (D+1)^2 get zeros)
 * Every output is written completely; Gaussians the forward culled get zeros.  dL_dscale / dL_drot are zero with
 * cov3D_precomp, dL_dsh is untouched with colors_precomp.
 *
 * The gradients are the reference's, including where its backward departs from the true derivative (straight-through
 * 0.99 alpha cap, 1e-7 in the conic inverse, no gradient through clamped tx / ty and clamped SH channels, the background
 * term; backward.cu:499, :203, :175-176, :32-34, :531-534), with one exception: dL_dscale carries the factor
 * scale_modifier, which the reference omits (backward.cu:321-325) -- identical at scale_modifier = 1.
 * The per-pixel contributions are summed WITHOUT float atomics (one row per (Gaussian, tile) instance, then a per-Gaussian
 * sum in a fixed order): two calls on the same state give bit-identical results.  The row buffer lives in the handle's
 * grow-only arenas (48 B per instance; gs2m_raster_backward_rows).
 *
 * Errors: no gs2m_rasterize_forward state in the handle (e.g. after gs2m_render_views), P / width / height different
 * from that call, GS2M_OPT_TILE_ROWS 2, GS2M_OPT_PAIR_BATCH > 1, an overflowed forward.  GS2M_OPT_EXACT_TILE_CULL 0 / 1 / 2
 * all work (a culled instance has alpha < 1/255 on its whole tile: zero gradient).  Synchronises the stream once (the
 * row count sizes the arena).
 *
 * STATED TOLERANCE: against an fp64 statement of the reference's forward differentiated by autograd
 * (tests/raster_statement.py; loss = sum(w * image), pixels with a threshold decision within 1e-4 excluded), every
 * gradient tensor is within 4 x the error of the SAME statement evaluated in fp32, in max|g - g64| / max|g64| and in
 * relative L2 (tests/test_raster_backward.py).  Measured on MI355X: e32 1e-6 .. 1.1e-5, the kernels at most 1.08 x e32
 * (profiles/raster_backward.txt).  The same bound holds PER GAUSSIAN (error of a Gaussian's gradient over its own largest
 * entry, floored at 1e-3 of the tensor's) on the designed edge cases of tests/test_raster_backward_edges.py: frustum clamp,
 * more than 65536 Gaussians, every SH degree with M above it, images below a tile, lists ending at the 64-instance batches,
 * saturation and the 0.99 cap; an entry whose sum is ill-conditioned is judged by the worst of several fp32 evaluations of
 * the statement instead, that entry alone (profiles/raster_backward_edges.txt).  SH coefficients above (D + 1)^2 are neither read nor given a gradient
 * other than zero, whatever they hold.
 */
int gs2m_rasterize_backward(gs2m_raster* r, int P, int D, int M, int R, const float* background,
                            int width, int height, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* scales, float scale_modifier,
                            const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                            const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                            const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                            float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                            float* dL_dscale, float* dL_drot, int debug, gs2m_stream stream);

/*
 * gs2m_rasterize_backward with gradients through the maps of gs2m_rasterize_depth as well (an extension, like the maps): the
 * argument list of gs2m_rasterize_backward with three upstream maps after dL_dpix.
 *
 *   dL_dpix[3,H,W]             device or NULL
 *   dL_ddepth_expected[H,W]    device or NULL: gradient of the loss by depth_expected   (gD)
 *   dL_ddepth_median[H,W]      device or NULL: ... by depth_median                     (gM)
 *   dL_dalpha[H,W]             device or NULL: ... by alpha                            (gA)
 * NULL means a map of zeros.  With the three new maps NULL (and dL_dpix given) the call IS gs2m_rasterize_backward: the same
 * kernels, bit-identical outputs.
 *
 * Per pixel, with the walk of gs2m_rasterize_depth (w_j = alpha_j T_j, S = sum w_j, Z = sum w_j z_j, T_f the final
 * transmittance, D = S > 0 ? Z / S : 0, A = 1 - T_f, med = z_m):
 *   - depth_expected is one more "colour channel" over a zero background with the per-instance value
 *     u_j = (gD / S)(z_j - D), 0 where S == 0: it adds T_j (u_j - rec_j) to dL/dalpha_j, rec being the reference's
 *     behind-the-contributor recurrence (backward.cu:515);
 *   - alpha: dA/dalpha_j = T_f / (1 - alpha_j), the shape of the background term (bg . dL_dpix becomes bg . dL_dpix - gA);
 *   - dL/dz_j: every contributing pixel adds w_j gD / S, the pixel whose median is instance j also adds gM.  depth_median is
 *     piecewise constant in everything but z_m: that is its stated derivative.  z_j is the view-space z of the centre, so
 *     dL_dmean3D receives (viewmatrix[2], viewmatrix[6], viewmatrix[10]) * sum dL/dz_j.
 * dL/dalpha_j continues into mean2D, conic and opacity exactly as for colour, under the same departures from the true
 * derivative (straight through the 0.99 cap, NDC-scaled mean2D, 1e-7 in the conic inverse, no gradient through clamped
 * tx / ty).  S, Z and the median are recomputed with the operations of gs2m_rasterize_depth: D has that call's bits and the
 * median is that call's instance.
 *
 * Preconditions, outputs, errors, arena (dL/dz_j is the tenth float of the 48-byte instance row) and the single stream
 * synchronisation are those of gs2m_rasterize_backward.  No float atomics: two calls give identical bits.
 *
 * STATED TOLERANCE: against the fp64 statement of gs2m_rasterize_backward's projection feeding the walk of
 * gs2m_rasterize_depth, differentiated by autograd (tests/depth_grad_statement.py; loss = sum(wC image + wD depth_expected +
 * wM depth_median + wA alpha), weights zero on pixels with a threshold decision within 1e-4, wM also where a transmittance is
 * within 1e-4 of 0.5), every gradient tensor is within 4 x the error of the SAME statement evaluated in fp32, in
 * max|g - g64| / max|g64| and in relative L2 (tests/test_raster_depth_backward.py), and per Gaussian on the designed edge
 * cases of tests/test_raster_depth_backward_edges.py.  Figures: profiles/raster_depth_backward.txt.
 */
int gs2m_rasterize_backward_depth(gs2m_raster* r, int P, int D, int M, int R, const float* background,
                                  int width, int height, const float* means3D, const float* shs,
                                  const float* colors_precomp, const float* scales, float scale_modifier,
                                  const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                  const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                  const float* dL_dpix, const float* dL_ddepth_expected,
                                  const float* dL_ddepth_median, const float* dL_dalpha, float* dL_dmean2D,
                                  float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                                  float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug,
                                  gs2m_stream stream);

/* Instance rows of the last gs2m_rasterize_backward call and the bytes of the row arena (0: never allocated). */
int gs2m_raster_backward_rows(gs2m_raster* r, int64_t* rows, int64_t* arena_bytes);

/*
 * Depth and opacity maps of the LAST gs2m_rasterize_forward on this handle.  An extension: the reference's renderCUDA writes
 * colour only.  One kernel walks the kept per-tile lists front to back with the alpha function of the backward pass
 * (csrc/raster_depth.h) and takes renderCUDA's three decisions per pixel.  Per pixel, T = 1, S = 0, Z = 0, med = 0; for every
 * instance j of the tile's list in order:
 *     skip j if power > 0 or alpha < 1/255, with alpha = min(0.99, o G)
 *     T' = T (1 - alpha); if T' < 1e-4 the pixel is finished, BEFORE accumulating (forward.cu:345-350)
 *     S = fma(T, alpha, S);  w = alpha T (rounded);  Z = fma(w, z_j, Z);  T = T';   if med == 0 and T <= 0.5: med = z_j
 * z_j is the view-space z of the Gaussian's CENTRE (the depth of the sort key), not a ray-surface intersection.
 *
 *   depth_expected[H,W]  device or NULL: S > 0 ? Z / S : 0    (alpha-weighted mean z of the contributors)
 *   depth_median[H,W]    device or NULL: med                  (z of the contributor that takes T to 0.5 or below)
 *   alpha[H,W]           device or NULL: 1 - T                (the forward's image is C + (1 - alpha) bg)
 * Every non-NULL output is written completely, with plain stores, each pixel once: two calls give identical bits.  A pixel
 * without a contributor holds exactly 0 in all three; listed Gaussians have z > 0.2, so 0 means "no depth" (what the TSDF
 * integrator treats as invalid).  1 - T is exact for T in [0.5, 1]: depth_median > 0 exactly where alpha >= 0.5.  The handle's
 * state is only read: a gs2m_rasterize_backward may follow.  Gradients through these maps: gs2m_rasterize_backward_depth.
 *
 * Errors, as gs2m_rasterize_backward: no gs2m_rasterize_forward state in the handle (e.g. after gs2m_render_views or
 * gs2m_raster_reserve), width / height different from that call, GS2M_OPT_TILE_ROWS 2, GS2M_OPT_PAIR_BATCH > 1, an overflowed
 * forward.  GS2M_OPT_EXACT_TILE_CULL 0 / 1 / 2 give the same bits (a culled instance has alpha < 1/255 on its whole tile).
 * Asynchronous, no host wait: the overflow flag is the forward's host-mapped status word as it stands, i.e. current once
 * the stream has been synchronised after the forward (gs2m_raster_status does); the kernel clamps every list range to the
 * arena, so a call on an overflow not yet visible reads nothing out of bounds and its maps are as invalid as the image.
 *
 * STATED TOLERANCE: against an fp64 statement of the walk above (tests/depth_statement.py), on pixels without a threshold
 * decision within 1e-4 and without a transmittance within 1e-4 of 0.5, alpha and depth_expected are within 4 x the error of
 * the SAME statement evaluated in fp32, in max|x - x64| / max|x64| and in relative L2, and depth_median is bit-equal to the
 * fp32 view-space z of the statement's median Gaussian (tests/test_raster_depth.py; figures: profiles/raster_depth.txt).
 */
int gs2m_rasterize_depth(gs2m_raster* r, int width, int height, float* depth_expected, float* depth_median,
                         float* alpha, gs2m_stream stream);

/*
 * The maps of gs2m_rasterize_depth with the RAY-GAUSSIAN INTERSECTION depth of every (instance, pixel) where that call has the
 * z of the centre (csrc/raster_depth_ray.h).  The centre's z is wrong wherever a surface is not fronto-parallel: a flat
 * Gaussian on a tilted surface covers pixels whose rays meet it nearer or farther than its centre, and the map is a staircase.
 * Produces the maps of the LAST gs2m_rasterize_forward on this handle, whose inputs P, means3D, scales, scale_modifier,
 * rotations, viewmatrix, tanfovx, tanfovy, width and height must be (the convention of gs2m_rasterize_backward).
 *
 * For Gaussian j: W = the upper 3 x 3 of the view matrix as computeCov2D reads it (W[i][k] = viewmatrix[4 k + i]), mu = its
 * view-space mean (transformPoint4x3), s = scale_modifier * scales[j], R(q) = the rotation matrix as computeCov3D forms it from
 * rotations[j], used as given (unit quaternions are assumed), M = W R.  The maximum of the Gaussian's density along the pixel's
 * ray x = t r (r_z = 1, so t is a view-space depth) is t* = (r^T B mu) / (r^T B r) for B ANY positive multiple of
 * adj(Sigma_view); the adjugate exists for a singular Sigma, so a disc of zero thickness gives exactly the ray-plane
 * intersection (n . mu) / (n . r).  In factors, without cancellation between terms and without 2 x 2 minors:
 *     g = (s1 s2, s0 s2, s0 s1);  gmax = max g_k
 *     if !(gmax > 0) or gmax not finite:  w_k = 0, c_k = 0      (rank <= 1: no orientation)
 *     else  w_k = (g_k / gmax) * (column k of M),  c_k = w_k . mu        k = 0, 1, 2
 *     sz  = sqrt(max(sum_k s_k^2 M[2][k]^2, 0))     (fmaxf semantics: a NaN counts as 0)
 *     lo  = max(z_c - 4 sz, 0.2),  hi = z_c + 4 sz   (z_c = the view depth of the forward's record, the sort key's)
 * and per (instance, pixel), px, py the integer pixel coordinates:
 *     r   = (((2 px + 1) / W - 1) tanfovx, ((2 py + 1) / H - 1) tanfovy, 1)     (the inverse of ndc2Pix: pixel centres at integers)
 *     u_k = w_k . r;  num = sum_k c_k u_k;  den = sum_k u_k^2
 *     t   = (den > 0 and num / den is finite) ? num / den : z_c
 *     z_j(p) = min(max(t, lo), hi)
 * The walk is that of gs2m_rasterize_depth, unchanged -- the same alpha, the same three decisions, the same S / Z / median rule
 * -- with z_j(p) where z_j stood: Z = fma(w, z_j(p), Z), and the median is z_j(p) of the first contributor that takes T to 0.5
 * or below.  The clamp is exact for every ray that passes within 4 sigma of the centre (the maximum along such a ray lies inside
 * that ellipsoid); it bounds what an edge-on disc, visible only through the 0.3 px dilation, can contribute.  By construction
 * every z_j(p) is finite and in [lo, hi] within [0.2, inf) for a finite z_c, 0 still means "no depth", and alpha does not depend
 * on z at all: it has the bits of gs2m_rasterize_depth's alpha, and depth_median > 0 exactly where alpha >= 0.5.
 * An isotropic Gaussian carries no surface orientation: its t* is the point of the ray nearest the centre, (mu . r) / (r . r),
 * which is no better a surface estimate than the centre's z.  The gain is for flat Gaussians.
 *
 *   depth_expected[H,W], depth_median[H,W], alpha[H,W]   device or NULL, as gs2m_rasterize_depth; all NULL does nothing
 * Every non-NULL output is written completely with plain stores: two calls give identical bits.  Asynchronous, no host wait
 * (the first call, and a call with a larger P than any before, allocate the handle's [P] 64-byte ray records).  Only the forward
 * state is read: a gs2m_rasterize_backward or gs2m_rasterize_depth may follow and gives the bits it gives without this call.
 * No gradients flow through these maps.
 *
 * Errors: those of gs2m_rasterize_depth (no forward state, width / height mismatch, GS2M_OPT_TILE_ROWS 2,
 * GS2M_OPT_PAIR_BATCH > 1, an overflowed forward); P different from the forward's; NULL means3D / scales / rotations /
 * viewmatrix.  A forward that took cov3D_precomp has no ray depth (the adjugate by minors cancels exactly where it matters:
 * on flat Gaussians): pass scales and rotations to both.
 *
 * STATED TOLERANCE: against an fp64 statement of the definition above on the walk of tests/depth_statement.py
 * (tests/ray_depth_statement.py), on the pixels gs2m_rasterize_depth's tolerance keeps and where no contributor's ray lies
 * within about 1.8 degrees of its Gaussian's plane (den / (sum_k |w_k|^2 |r|^2) < 1e-3: num / den loses its digits in fp32),
 * depth_expected, and depth_median against z_j(p) of the statement's median Gaussian, are within 4 x the error of the SAME
 * statement evaluated in fp32 plus (8 + 2 sqrt(n)) 2^-24 (n = the longest run of contributors), in max|x - x64| / max|x64| and
 * in relative L2 (tests/test_raster_depth_ray.py, tests/test_raster_depth_ray_edges.py; figures:
 * profiles/raster_depth_ray.txt).
 */
int gs2m_rasterize_depth_ray(gs2m_raster* r, int P, const float* means3D, const float* scales, float scale_modifier,
                             const float* rotations, const float* viewmatrix, float tanfovx, float tanfovy,
                             int width, int height, float* depth_expected, float* depth_median, float* alpha,
                             gs2m_stream stream);

/*
 * Backward of the LAST gs2m_rasterize_forward on this handle with gradients through the maps of gs2m_rasterize_depth_ray: the
 * argument list of gs2m_rasterize_backward_depth, the three upstream maps being those of the ray maps.  The alpha path is
 * that call's, with z_j(p) of the ray forward (recomputed by the forward's own function: D and the median instance have the
 * bits of gs2m_rasterize_depth_ray) where it has z_j:  u_j = (gD / S)(z_j(p) - D).
 *
 * What is new is where h = dL/dz_j(p) goes (per instance j and pixel p, h = w_j gD / S, plus gM on the pixel whose median is
 * j).  In the notation of gs2m_rasterize_depth_ray, r = (rx, ry, 1), u_k = w_k . r, num = sum c_k u_k, den = sum u_k^2:
 *   - t = num / den taken and lo <= t <= hi:  dt/dc_k = u_k / den,  dt/dw_k = ((c_k - 2 t u_k) / den) r.  Summed over the
 *     pixels these are ten moments  A = sum (h / den) r  and  Bm = sum (h t / den) r r^T (symmetric), and
 *         dL/dc_k = w_k . A,    dL/dw_k = c_k A - 2 Bm w_k;
 *   - the fallback (den > 0 false or a non-finite quotient: t = z_c): h goes to dL/dz_c;
 *   - t > hi, or t < lo with lo = z_c - 4 sz: h goes to dL/dz_c and +4 h (hi) or -4 h (lo) to dL/dsz -- the derivative of the
 *     clamp as stated;
 *   - t < lo with lo the 0.2 floor: no gradient.
 * Then, per Gaussian: c_k = w_k . mu (to w_k and mu);  w_k = (g_k / gmax) M[:,k], g = (s1 s2, s0 s2, s0 s1), differentiated
 * THROUGH gmax.  (t is invariant under a common scaling of all (w_k, c_k), so holding gmax constant is the same gradient in
 * exact arithmetic; through gmax the derivative by the largest g_k, the remainder of two sums that cancel, is never formed.)
 * sz = sqrt(sum_k s_k^2 M[2][k]^2) to s and row 2 of M, the derivative through the square root taken as 0 where the sum is 0;
 * mu and z_c to dL_dmean3D through the view rotation;  M = W R(q) to dL_drot with q as given, as computeCov3D's backward
 * treats it;  s = scale_modifier * scales to dL_dscale, which keeps the factor scale_modifier as in gs2m_rasterize_backward.
 * The three results are ADDED to what the colour / alpha path writes into dL_dmean3D, dL_dscale and dL_drot.  A centre
 * depth can only push a Gaussian along the view axis; this derivative also turns it.
 *
 * With dL_ddepth_expected and dL_ddepth_median both NULL no depth is read: the call IS gs2m_rasterize_backward_depth, bit for
 * bit.  Preconditions and errors: those of gs2m_rasterize_backward_depth and of gs2m_rasterize_depth_ray -- cov3D_precomp
 * non-NULL, or NULL scales or rotations, is an error; on an error nothing is written.  One stream synchronisation.  The ten
 * moments and dL/dsz are a second 48-byte row per instance, in an arena of their own that only this entry allocates; no
 * float atomics, every sum in a fixed order: two calls give identical bits.
 *
 * STATED TOLERANCE: against the fp64 statement tests/ray_depth_grad_statement.py (tests/depth_grad_statement.py with z_j(p)
 * of tests/ray_depth_statement.py over leaf tensors), weights zero as for gs2m_rasterize_backward_depth and also on grazing
 * pixels (gs2m_rasterize_depth_ray's 1e-3) and where a contributor's t lies within 1e-4 relative of lo or hi, every gradient
 * tensor is within 4 x the error of the SAME statement evaluated in fp32, in max|g - g64| / max|g64| and in relative L2
 * (tests/test_raster_depth_ray_backward.py, tests/test_raster_depth_ray_backward_edges.py; figures:
 * profiles/raster_depth_ray_backward.txt).
 */
int gs2m_rasterize_backward_depth_ray(gs2m_raster* r, int P, int D, int M, int R, const float* background,
                                      int width, int height, const float* means3D, const float* shs,
                                      const float* colors_precomp, const float* scales, float scale_modifier,
                                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                      const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                      const float* dL_dpix, const float* dL_ddepth_expected,
                                      const float* dL_ddepth_median, const float* dL_dalpha, float* dL_dmean2D,
                                      float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                                      float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug,
                                      gs2m_stream stream);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:26-31,
 * rasterizer_impl.cu:54-66,141-153).  present[P]: device, 1 byte per Gaussian. */
int gs2m_mark_visible(int P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present, gs2m_stream stream);

/* Host-side camera record = the per-view fields of GaussianRasterizationSettings
 * (DGR/diff_gaussian_rasterization/__init__.py:157-169).  Matrices in the same
 * transposed row-major layout the reference passes. */
typedef struct gs2m_camera {
    int32_t width, height;
    float tanfovx, tanfovy;
    float viewmatrix[16];
    float projmatrix[16];
    float campos[3];
} gs2m_camera;

/* Gaussian store handed to the pipeline-level entry point.  `raw` != 0 means the arrays
 * hold the GaussianModel's pre-activation parameters (GS/scene/gaussian_model.py:95-115):
 * log-scales, unnormalised quaternions, logit opacities; exp / normalize / sigmoid are
 * fused into the projection kernel.  shs is [P,M,3] (get_features layout) or, when
 * shs_rest != NULL, shs = features_dc [P,1,3] and shs_rest = features_rest [P,M-1,3]
 * (saves the torch.cat of GS/scene/gaussian_model.py:108-111). */
typedef struct gs2m_gaussians {
    int32_t P, sh_degree, M, raw;
    const float* xyz;       /* [P,3] */
    const float* scales;    /* [P,3] */
    const float* rotations; /* [P,4] wxyz */
    const float* opacities; /* [P]   */
    const float* shs;       /* [P,M,3] or features_dc [P,1,3] */
    const float* shs_rest;  /* NULL or features_rest [P,M-1,3] */
} gs2m_gaussians;

/*
 * Pipeline-level entry point: renders n_views views (a stereo pair = 2) of the same
 * Gaussians in one fused pass.  Replaces the per-eye loop of Renderer.render_image_pair
 * (gs2mesh_utils/renderer_utils.py:378-389) -> render() (GS/gaussian_renderer/__init__.py:18-100)
 * -> rasterizer.  cams and bg are HOST pointers (copied at call time).
 *   out_color  [n_views,3,H,W] f32 device, or NULL
 *   out_rgb8   [n_views,H,W,3] u8 device, or NULL: saturate(rint(255*c)), the conversion
 *              cv2.imwrite applies to the float image (renderer_utils.py:389-390)
 *   out_radii  [n_views,P] i32 device, or NULL
 * All views must share width/height.  Asynchronous; same arena/overflow contract as
 * gs2m_rasterize_forward.
 *
 * STATED TOLERANCE against the reference rasteriser (DGR/cuda_rasterizer/forward.cu:261-374) on identical inputs; the same
 * statement holds for gs2m_rasterize_forward.  Projection, instance lists and sort order are exact (record, point_list,
 * ranges, radii, num_rendered bit-identical at the defaults).  The compositing stage evaluates alpha in the log2 domain
 * (v_exp_f32, 1 ulp) and accumulates rgb * (T - T'), so:
 *   - on every pixel where NO decision of renderCUDA (power > 0, alpha < 1/255, T' < 1e-4) is taken within a relative
 *     band of 1e-5 of its threshold, |out_color - reference| <= 2e-4 per value ("clean bar");
 *     measured <= 5.5e-7 on C2 .. C5 (profiles/r4_parity_*.json);
 *   - elsewhere a decision may flip; the difference is then bounded by 2e-4 + the contribution of the flipped
 *     instances (oracle/parity.py:flip_attribution computes that bound per pixel; the tests assert zero unexplained
 *     pixels).  Measured global maxima: 2.0e-3 on C2 (25 k of 3.84 M pixels carry a candidate flip), 3.8e-4 on C3,
 *     3.8e-3 on C4, 6.2e-4 on C5; the tests bound them by <= 2x measured (tests/test_fullsize_gpu.py:BENCH_PARITY_BOUNDS);
 *   - out_rgb8 differs from the quantised reference by at most 1 LSB, on <= 70 pixels of a C2 eye;
 *   - with g->raw != 0 (activations fused into the projection: exp / sigmoid / normalize in device arithmetic, 1 ulp from
 *     numpy's) about 1 radius in 3e5 Gaussians moves by one pixel and one (Gaussian, tile) instance with it; the
 *     bench line and the tests report the count (`radii_mismatches`), the image bound above already includes it.
 */
int gs2m_render_views(gs2m_raster* r, const gs2m_gaussians* g, const gs2m_camera* cams,
                      int n_views, const float* bg /* host[3] */, float scale_modifier,
                      float* out_color, uint8_t* out_rgb8, int* out_radii, gs2m_stream stream);

/*
 * Optional one-time preparation for gs2m_render_views (Renderer.prepare_renderer stage): keeps a
 * wave-transposed copy of the SH block ([P/64][12][64] float4, +192 B per Gaussian) inside the handle.
 * Later gs2m_render_views calls whose gs->shs / shs_rest / P match read that copy with fully
 * coalesced loads; the caller's arrays must not change in between (call again after an update;
 * a call with P == 0 or M != 16 just drops the copy).  Same results either way.
 */
int gs2m_raster_pack_sh(gs2m_raster* r, const gs2m_gaussians* g, gs2m_stream stream);

/*
 * Superset of gs2m_raster_pack_sh (same stage, same matching rule, extended to xyz / scales / rotations /
 * opacities): keeps a SPATIALLY ORDERED packed copy of the whole model inside the handle (+236 B per Gaussian).
 * order[P] (device, int32) is a permutation: position j of the copy holds Gaussian order[j] -- e.g. the Morton
 * order of xyz (gs2mesh_amd.rasterizer.morton_order).  A trained splat is stored in densification order
 * (GS/scene/gaussian_model.py:372-409 appends clones and splits), i.e. spatially random: every workgroup of the
 * counting sort then touches every tile.  In a spatially ordered copy consecutive Gaussians project to a few
 * neighbouring tiles: the keys a workgroup scatters form long runs and the records a tile gathers lie close together.
 * Results are those of the unordered model: the sort keys carry the Gaussian IDS (ties in depth resolve in id order,
 * as the reference's stable sort does), out_radii and the parity taps are indexed by id.  Synchronises `stream` once
 * (the permutation is verified); returns an error if `order` is not a permutation.
 */
int gs2m_raster_pack_model(gs2m_raster* r, const gs2m_gaussians* g, const int32_t* order /* device [P] */,
                           gs2m_stream stream);

/* The packed copies are matched to the caller's arrays by DEVICE POINTER (and P) only: after an in-place update of any
 * Gaussian parameter, or when tensors may have been freed and re-allocated at the same addresses, call this (or pack
 * again) -- later gs2m_render_views calls then read the caller's arrays until the next pack. */
int gs2m_raster_pack_invalidate(gs2m_raster* r);

/* Synchronises `stream` (pass the stream the handle is used on) and reports num_rendered[v] for
 * v < n_views of the LAST forward/render_views call on the handle (host array, may be NULL), and
 * whether the instance arena overflowed in ANY call since the previous status query
 * (*overflow = 1: the images of the overflowing calls are invalid; *required = the largest
 * per-view instance count any of those calls needed).  The overflow word is sticky on the device:
 * a later call that fits does not erase it; this query consumes it. */
int gs2m_raster_status(gs2m_raster* r, gs2m_stream stream, int n_views,
                       int64_t* num_rendered, int* overflow, int64_t* required);

/* With GS2M_OPT_STAGE_TIMING on: synchronises `stream`, then adds the hipEvent-measured
 * GPU time of every stage launch recorded since the last query to total_ms[GS2M_N_STAGES]
 * and the number of launches to launches[GS2M_N_STAGES] (host arrays, caller-zeroed). */
int gs2m_raster_stage_times(gs2m_raster* r, gs2m_stream stream, double* total_ms,
                            int64_t* launches);

/* Phase profile of the compositing kernel (GS2M_OPT_BLEND_PROFILE 1): synchronises `stream`, copies the counters summed
 * over every wave launched since the last query to counters[GS2M_BLEND_PROF_COUNTERS] (host) and clears them:
 *   [0] waves  [1] wave lifetime  [2] waiting for the record DMA  [3] staging a batch (transform, cull, compaction)
 *   [4] issuing the next batch's loads  [5] compositing loop  [6] epilogue (background, image stores)   -- shader cycles
 *   [7] staged batches  [8] staged instances (after the per-half / finished-quadrant cull)  [9] listed instances
 * The stamps themselves cost ~10 % of the wave's cycles: read the counters as shares. */
#define GS2M_BLEND_PROF_COUNTERS 10
int gs2m_raster_blend_cycles(gs2m_raster* r, gs2m_stream stream, uint64_t* counters);

/* Debug/parity taps: copy the projected per-Gaussian record of view `v` of the last call to
 * HOST buffers (any may be NULL): means2D[P,2], depths[P], conic_opacity[P,4], rgb[P,3],
 * rect[P,4] (u16 x0,y0,x1,y1), tiles_touched[P].  Synchronises. */
int gs2m_raster_download_geometry(gs2m_raster* r, gs2m_stream stream, int v, int P,
                                  float* means2D, float* depths, float* conic_opacity,
                                  float* rgb, uint16_t* rect, uint32_t* tiles_touched);
/* Copy view v's sorted instance list and tile ranges to HOST: point_list[n] (Gaussian ids,
 * n = num_rendered[v]), ranges[tiles,2].  Synchronises. */
int gs2m_raster_download_binning(gs2m_raster* r, gs2m_stream stream, int v, int64_t n,
                                 uint32_t* point_list, int32_t n_tiles, uint32_t* ranges);

/* ------------------------------------------------------------------------------------ */
/* TSDF fusion                                                                          */
/* ------------------------------------------------------------------------------------ */

typedef struct gs2m_tsdf gs2m_tsdf;

enum { GS2M_TSDF_COLOR_NONE = 0, GS2M_TSDF_COLOR_RGB8 = 1 };

/*
 * Replaces open3d.pipelines.integration.ScalableTSDFVolume(voxel_length, sdf_trunc,
 * color_type[, volume_unit_resolution=16, depth_sampling_stride=4]) as constructed at
 * gs2mesh_utils/tsdf_utils.py:53-56 (Open3D 0.17.0, requirements.txt:15; the C++ is not
 * in the reference tree -- algorithm restated in oracle/tsdf_oracle.cpp).
 * max_blocks = capacity of the 16^3-voxel block pool (20 B/voxel = 80 KiB per block).
 */
int gs2m_tsdf_create(gs2m_tsdf** out, double voxel_length, double sdf_trunc, int color_type,
                     int volume_unit_resolution, int depth_sampling_stride, int64_t max_blocks,
                     int device);
int gs2m_tsdf_destroy(gs2m_tsdf* t);
int gs2m_tsdf_reset(gs2m_tsdf* t, gs2m_stream stream);

/*
 * Replaces RGBDImage.create_from_color_and_depth(color, depth, depth_scale, depth_trunc,
 * convert_rgb_to_intensity=False) + PinholeCameraIntrinsic(w,h,fx,fy,cx,cy) +
 * volume.integrate(rgbd, intrinsic, extrinsic)  (tsdf_utils.py:88-93,106-107).
 *   depth   [H,W] f32 device (raw: the kernel applies d/depth_scale, d >= depth_trunc -> 0)
 *   color   [H,W,3] u8 device (may be NULL when color_type == NONE)
 *   mask    [H,W] u8 device or NULL: depth is multiplied by (mask != 0) first
 *           (tsdf_utils.py:68-81 object/occlusion masks)
 *   min_depth: depth < min_depth -> 0 before scaling (tsdf_utils.py:83); pass 0 to skip
 *   extrinsic_w2c: HOST, row-major 4x4 float64 world->camera (what the reference passes:
 *           np.linalg.inv(extrinsic_matrix)); a singular matrix is an error
 * Depths that are not positive after the conversion -- zero, negative, NaN (also NaN * mask), -inf, and +inf under any
 * depth_trunc, the default inf included (+inf >= inf) -- touch no block and update no voxel, as in Open3D.  The 64 strided
 * pixels one wavefront of the touch pass handles must span at most 2^24 blocks (the box around all their +-sdf_trunc
 * cubes): a wider span is not integrated but refused with overflow flag 4, like a block index outside the key range
 * (tests/test_tsdf_edges.py).
 * Asynchronous.
 */
int gs2m_tsdf_integrate(gs2m_tsdf* t, const float* depth, const uint8_t* color,
                        const uint8_t* mask, int width, int height, double fx, double fy,
                        double cx, double cy, const double* extrinsic_w2c, double depth_scale,
                        double depth_trunc, double min_depth, gs2m_stream stream);

/*
 * The same for n_frames frames of one size / intrinsics in ONE sweep over the touched blocks (SURVEY.md 7 step 6 iii):
 * every block keeps its voxels in registers while the frames that touch it are applied IN FRAME ORDER, so the result is
 * bit-identical to n_frames gs2m_tsdf_integrate calls in that order, with one state read + write per batch instead of
 * per frame.  depth / color / mask: HOST arrays of n_frames DEVICE pointers (mask may be NULL, or hold NULLs);
 * extrinsics_w2c: HOST [n_frames][16].  Batches of up to 64 frames per sweep (longer lists are split).  Asynchronous; the
 * images must stay valid until the stream reaches the end of the call.
 */
int gs2m_tsdf_integrate_batch(gs2m_tsdf* t, int n_frames, const float* const* depth, const uint8_t* const* color,
                              const uint8_t* const* mask, int width, int height, double fx, double fy, double cx,
                              double cy, const double* extrinsics_w2c, double depth_scale, double depth_trunc,
                              double min_depth, gs2m_stream stream);

/* Stage timing as for the rasteriser: enable != 0 brackets k_tsdf_touch (index 0) and
 * k_tsdf_integrate (index 1) with hipEvents; gs2m_tsdf_stage_times synchronises and
 * accumulates into total_ms[2] / launches[2]. */
int gs2m_tsdf_set_stage_timing(gs2m_tsdf* t, int enable);   /* a batch counts as n_frames launches of each stage */
int gs2m_tsdf_stage_times(gs2m_tsdf* t, gs2m_stream stream, double* total_ms, int64_t* launches);

/* Synchronises; n_blocks = allocated blocks, block_updates = sum over frames of blocks
 * integrated (x 4096 = voxel-updates), overflow = flag bits (0 = fine): 1 block pool exhausted, 2 hash table full,
 * 4 block index outside the +-2^20 key range, 8 a voxel handed to gs2m_tsdf_pack(GS2M_XFORM_SUM_PACKED) did not fit the
 * packed fields (weight > 1023 or a colour sum >= 2^18: the summed exchange buffers are invalid, use SUM_F32). */
int gs2m_tsdf_status(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_blocks,
                     int64_t* block_updates, int* overflow);

/* The overflow flag word of gs2m_tsdf_status (bits 1 / 2 / 4 / 8) copied to a DEVICE word, asynchronously: lets a multi-GPU
 * caller all-reduce the verdict of a pack on the device and pay ONE host read for it (gs2mesh_amd.parallel.reduce_volume)
 * instead of a status synchronisation followed by the read of the reduced flag. */
int gs2m_tsdf_flags_device(gs2m_tsdf* t, uint32_t* flags_dev, gs2m_stream stream);

/* Copy allocated blocks to HOST (any pointer may be NULL): keys[n,3] (block index),
 * tsdf[n,4096], weight[n,4096] (voxel x*256+y*16+z, Open3D IndexOf), rgb_sum[n,4096,3] u32
 * (sum of u8 colours; mean colour = rgb_sum/weight).  n must be >= n_blocks. Synchronises. */
int gs2m_tsdf_download(gs2m_tsdf* t, gs2m_stream stream, int64_t n, int32_t* keys,
                       float* tsdf, float* weight, uint32_t* rgb_sum);

/* Block keys of the first n allocated blocks to a DEVICE buffer keys[n,3] (i32), in slot order.  Halo copies (blocks of
 * another rank brought in by gs2m_tsdf_unpack(..., halo = 1)) are reported as the out-of-range sentinel key
 * (2^20 - 1 in every component): they are not this volume's to exchange. */
int gs2m_tsdf_block_keys(gs2m_tsdf* t, int64_t n, int32_t* keys, gs2m_stream stream);

/*
 * Multi-GPU exchange (new; the reference is single-GPU).  pack_sum: for the n canonical block keys (device [n,3])
 * write this volume's accumulators in SUM form to ONE device buffer buf[n,5,4096] of fp32 planes
 * {wsum = tsdf*weight, weight, sum r, sum g, sum b} (zeros where the block is not allocated here).  Counts and colour
 * sums are integers < 2^24, exact in fp32: the host reduces the whole buffer with a single RCCL collective
 * (reduce-scatter or all-reduce), then unpack_sum replaces the state of the listed blocks (allocating as needed)
 * with tsdf = wsum/weight.  halo != 0 marks the blocks as neighbour-only: gs2m_tsdf_extract reads them for the +1
 * corners of its cubes but starts no cube in them (the rank that owns them does): owner-side mesh extraction.
 */
int gs2m_tsdf_pack_sum(gs2m_tsdf* t, const int32_t* keys, int64_t n, float* buf, gs2m_stream stream);
int gs2m_tsdf_unpack_sum(gs2m_tsdf* t, const int32_t* keys, int64_t n, const float* buf, int halo,
                         gs2m_stream stream);

/*
 * Block-map key exchange (multi-GPU): the union of the ranks' block sets as a dense map over a WINDOW of
 * block indices lo[k] <= b[k] < lo[k] + dim[k] (host int32[3] each; the same on every rank).  SURVEY asks for a bitmap under a
 * bitwise OR; RCCL has no bitwise reduction, so the map holds one BYTE per block and the caller's collective is MAX over uint8.
 *   gs2m_tsdf_map_bytes    bytes of the exchange buffer: the cells (dim0 * dim1 * dim2 rounded up to 16)
 *                          + GS2M_TSDF_MAP_HEADER_BYTES + 8 * world header bytes (-1: bad window).
 *   gs2m_tsdf_block_map    clears `cells` (device, 16-byte aligned) and marks this rank's blocks (halo copies are not its
 *                          blocks); the header behind the cells carries, in a form a bytewise MAX reduces: [0] a block outside the
 *                          window, [1..4] the volume's overflow flags 1 / 2 / 4 / 8, [5] / [6] bits 0 / 1 of `flags` (caller-defined),
 *                          [8..11] / [12..15] the bytes of max_blocks and of its complement (byte + complement byte == 255 after
 *                          the MAX <=> the ranks agree), [16..23] the same for a hash of the window, [32 + 8 r ..] frames_local and
 *                          frames_base of rank r as little-endian u32 (zeros in the other ranks' slots).  Asynchronous, no host
 *                          read.  The caller all-reduces the buffer with MAX.
 *   gs2m_tsdf_map_keys     on the reduced buffer: marked cells -> keys[n][3] (device) in cell order = ascending (x, y, z), the
 *                          canonical order of the exchange, identical on every rank; header bytes [24..27] = n (keys beyond
 *                          max_keys are counted, not written); copies the header to header_host[GS2M_TSDF_MAP_HEADER_BYTES + 8 * world]
 *                          and synchronises -- the one host read of the key exchange.
 * Replaces round 4's "gather every rank's key list, sort, unique" (gs2mesh_amd/parallel.py keeps it as the fallback for blocks
 * outside the window).
 */
#define GS2M_TSDF_MAP_HEADER_BYTES 32
int64_t gs2m_tsdf_map_bytes(const int32_t* dim, int world);
int gs2m_tsdf_block_map(gs2m_tsdf* t, const int32_t* lo, const int32_t* dim, int rank, int world, int64_t frames_local,
                        int64_t frames_base, int flags, uint8_t* cells, gs2m_stream stream);
int gs2m_tsdf_map_keys(gs2m_tsdf* t, const int32_t* lo, const int32_t* dim, int world, uint8_t* cells, int32_t* keys,
                       int64_t max_keys, uint8_t* header_host, gs2m_stream stream);

/* The same with a choice of exchange form (pack_sum / unpack_sum = form GS2M_XFORM_SUM_F32):
 *   GS2M_XFORM_SUM_F32     buf_f32[n,5,4096] in SUM form as above (one fp32 SUM collective), buf_i64 unused;
 *   GS2M_XFORM_RAW_F32     buf_f32[n,5,4096] with the planes verbatim {tsdf, weight, sum r, sum g, sum b}: for copies of blocks
 *                          that are already reduced (halo exchange) -- no tsdf * w / w round trip, seam voxels bit-identical;
 *   GS2M_XFORM_SUM_PACKED  buf_f32[n,4096] = wsum, buf_i64[n,4096] = weight | sum r << 10 | sum g << 28 | sum b << 46: an fp32 SUM
 *                          and an int64 SUM collective, 12 instead of 20 bytes per voxel.  Only valid while the volumes being
 *                          summed have integrated <= 1023 frames IN TOTAL (weight < 2^10, colour sums < 2^18: no carry between
 *                          the fields); the caller checks that bound (gs2mesh_amd.parallel does, and falls back to SUM_F32);
 *                          a LOCAL value that does not fit its field raises status bit 8 (gs2m_tsdf_status).
 * Halo copies held by the volume are packed as zeros in the SUM forms (they are another rank's blocks). */
enum { GS2M_XFORM_SUM_F32 = 0, GS2M_XFORM_RAW_F32 = 1, GS2M_XFORM_SUM_PACKED = 2 };
int gs2m_tsdf_pack(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, float* buf_f32, int64_t* buf_i64,
                   gs2m_stream stream);
int gs2m_tsdf_unpack(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, const float* buf_f32,
                     const int64_t* buf_i64, int halo, gs2m_stream stream);
/* gs2m_tsdf_reset + gs2m_tsdf_unpack(halo = 0) of n DISTINCT in-range keys in one call, without writing the reduced blocks' bytes
 * twice: the reset leaves the voxel state of the first n slots alone (the unpack overwrites exactly those), and clears the rest
 * of the slots that were in use.  The tail of the multi-GPU reduction (gs2mesh_amd.parallel.reduce_volume). */
int gs2m_tsdf_replace(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, const float* buf_f32, const int64_t* buf_i64,
                      gs2m_stream stream);

/*
 * Replaces volume.extract_triangle_mesh() (tsdf_utils.py:108; Open3D ScalableTSDFVolume::
 * ExtractTriangleMesh): marching cubes over the allocated blocks; cubes with a zero-weight corner are
 * skipped, inside = tsdf < 0, vertices interpolated on the cut edges, vertex colour = interpolated
 * mean colour / 255.  gs2m_tsdf_extract_count synchronises and returns the triangle count;
 * gs2m_tsdf_extract writes min(count, max_triangles) un-welded triangles to DEVICE buffers
 * vertices[n,3,3] and colors[n,3,3] (float64, colors may be NULL), asynchronously after its
 * own count pass.  Vertices shared by neighbouring triangles are bit-identical (weld on the host).
 */
int gs2m_tsdf_extract_count(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_triangles);
int gs2m_tsdf_extract(gs2m_tsdf* t, gs2m_stream stream, int64_t max_triangles, double* vertices,
                      double* colors, int64_t* n_triangles);
/* The same + edge_index[n,3,4] (int32, DEVICE, may be NULL): per emitted vertex Open3D's vertex key -- the global voxel
 * index of the lower corner of the cut edge and the edge's axis (ExtractTriangleMesh's `edge_index`).  Welding by this key
 * instead of by position reproduces Open3D's vertex set also where a tsdf value is exactly 0 (the vertices of up to
 * three cut edges then share one position and Open3D keeps them apart). */
int gs2m_tsdf_extract_indexed(gs2m_tsdf* t, gs2m_stream stream, int64_t max_triangles, double* vertices,
                              double* colors, int32_t* edge_index, int64_t* n_triangles);

/*
 * Device-side mesh post-processing.  volume.extract_triangle_mesh() (gs2mesh_utils/tsdf_utils.py:108) returns
 * an INDEXED mesh: Open3D welds the marching-cubes vertices through an edge -> vertex map while it extracts.
 *   gs2m_tsdf_extract_mesh   count + emit + weld on the device: the vertices are welded by Open3D's vertex identity (the cut edge:
 *                            global voxel index of its lower corner + axis), numbered by first appearance in the deterministic
 *                            emission order of gs2m_tsdf_extract_indexed (= what welding that soup on the host gives).  The mesh stays
 *                            in the handle; *n_vertices / *n_triangles size the caller's buffers.  Synchronises.
 *   gs2m_tsdf_mesh_copy      copies the cached mesh to the caller: vertices [nv][3] f64, colors [nv][3] f64 (zeros for a colourless
 *                            volume), edge_index [nv][4] i32, triangles [nt][3] i32.  Each destination may be NULL and may be a
 *                            HOST or a device pointer (the PLY writer wants it on the host; the clustering below on the device).
 *   gs2m_mesh_cluster        TriangleMesh::ClusterConnectedTriangles (tsdf_utils.py:133): triangles are connected when they share an
 *                            edge.  triangles [n][3] i32, labels [n] i32 and cluster_n_triangles [n] i64 (capacity n; the first
 *                            *n_clusters entries are written) are DEVICE pointers.  Clusters are numbered by their smallest triangle
 *                            index (the numbering of a sweep from triangle 0 upwards).  Lock-free union-find over an edge hash table.
 */
int gs2m_tsdf_extract_mesh(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_vertices, int64_t* n_triangles);
int gs2m_tsdf_mesh_copy(gs2m_tsdf* t, gs2m_stream stream, double* vertices, double* colors, int32_t* edge_index, int32_t* triangles);
int gs2m_mesh_cluster(int device, gs2m_stream stream, int64_t n_triangles, const int32_t* triangles, int32_t* labels,
                      int64_t* cluster_n_triangles, int64_t* n_clusters);
/*
 *   gs2m_mesh_vertex_normals TriangleMesh::ComputeVertexNormals (tsdf_utils.py:110), bit-identical to the numpy statement of
 *                            gs2mesh_amd.mesh.TriangleMesh.compute_vertex_normals: triangle normal = np.cross(v1 - v0, v2 - v0)
 *                            divided by its norm sqrt((x*x + y*y) + z*z) (by 1 when that is 0); vertex normal = the sum, from
 *                            0.0, of the normals of the triangles that use it in np.add.at order (corner 0 of every triangle in
 *                            ascending triangle order, then corner 1, then corner 2), normalised the same way (0 without
 *                            triangles).  vertices [n_vertices][3] f64, triangles [n_triangles][3] i32, triangle_normals
 *                            [n_triangles][3] f64 and vertex_normals [n_vertices][3] f64 are DEVICE pointers.  A vertex index
 *                            outside 0..n_vertices-1 is an error.  Synchronises `stream` before it returns.
 */
int gs2m_mesh_vertex_normals(int device, gs2m_stream stream, int64_t n_vertices, const double* vertices, int64_t n_triangles,
                             const int32_t* triangles, double* triangle_normals, double* vertex_normals);

/* ------------------------------------------------------------------------------------ */
/* stereo post-processing (between the stereo network and the TSDF)                     */
/* ------------------------------------------------------------------------------------ */

/*
 * Replaces Stereo.get_occlusion_mask(disparity_LR, disparity_RL, stereo_occlusion_threshold) and
 * depth = fx * baseline / disparity_LR (gs2mesh_utils/stereo_utils.py:132-133,149-179), fused.
 *   disp_lr, disp_rl  [H,W] f32 device (disp_rl may be NULL when mask_out is NULL)
 *   depth_out         [H,W] f32 device or NULL
 *   mask_out          [H,W] u8 device or NULL: 1 = visible (the reference returns ~occlusion_mask)
 * With xp = (int32)(x - disp_lr[y][x]) truncated toward zero: a pixel whose x - disp_lr is NaN or outside int32 is occluded.
 * (A NaN in disp_rl compares false with every threshold, so it occludes none of the pixels that read it, as in the reference.)
 * The outputs are the `depth` / `mask` inputs of gs2m_tsdf_integrate.  Asynchronous.
 */
int gs2m_stereo_depth_occlusion(const float* disp_lr, const float* disp_rl, int width, int height,
                                double fx_times_baseline, double occlusion_threshold, float* depth_out,
                                uint8_t* mask_out, gs2m_stream stream);

/*
 * Replaces the object-mask preprocessing of TSDF.run (gs2mesh_utils/tsdf_utils.py:69-83) for n frames in one call.  Per frame:
 *   m = object_mask != 0, inverted if invert != 0;
 *   if erode != 0: m = erode_k2(close_k1(m)) -- cv2.MORPH_CLOSE with a closing_k x closing_k box of ones, then cv2.erode with an
 *                  erosion_k x erosion_k box; default anchor (window [x - k/2, x + k - 1 - k/2] in both axes) and default
 *                  border (every operation sees 1 outside the image when it erodes, 0 when it dilates);
 *   out = m & (occlusion_mask != 0), written as 0 / 1 bytes.
 * Bit-identical to gs2mesh_amd.tsdf_utils.preprocess_object_mask followed by the AND.  Any k >= 1 (also k > width or height);
 * k < 1 is an error.
 *   object_masks, occlusion_masks   host arrays [n] of [height][width] u8 DEVICE pointers (non-zero = true); either array or
 *                                   any entry may be NULL (that mask is absent: an absent object mask counts as all true)
 *   out_masks                       host array [n] of [height][width] u8 DEVICE pointers; entry i is written when frame i has
 *                                   an object or an occlusion mask, and may be NULL (not touched) when it has neither
 *   scratch                         DEVICE, 2 * n * height * ceil(width / 64) words; may be NULL when erode == 0 or no frame
 *                                   has an object mask
 * Asynchronous on `stream`.
 */
int gs2m_mask_preprocess(int n, int width, int height, const uint8_t* const* object_masks, const uint8_t* const* occlusion_masks,
                         int invert, int erode, int closing_k, int erosion_k, uint8_t* const* out_masks, uint64_t* scratch,
                         gs2m_stream stream);

/*
 * Binary dilation of n masks with a disk: the `binary_dilation(mask, disk(24))` with which the DTU evaluation's cull_scan
 * widens every view's object mask (evaluation/DTU/eval_code/evaluate_single_scene.py:80), i.e. scipy.ndimage.binary_dilation
 * with skimage's disk(r) footprint.  Defined bit for bit, per mask:
 *   in(y, x)  = mask[y][x] != 0 inside the image, 0 outside it;
 *   out(y, x) = OR over all integer (dy, dx) with dy * dy + dx * dx <= radius * radius of in(y + dy, x + dx).
 * radius = 0 is the identity (out = mask != 0).
 *   n, width, height        any n >= 0 (worked off in chunks of 32 masks), width and height >= 1
 *   masks                   host array [n] of [height][width] u8 DEVICE pointers (non-zero = set), none of them NULL
 *   radius                  0 .. 64
 *   out_bits                [n][height][nw] u64 device, nw = (width + 63) / 64: bit x & 63 of word x >> 6 is pixel x, the bits
 *                           at x >= width are 0.  This is the `mask_bits` of gs2m_points_cull_views.
 *   out_bytes               NULL, or [n][height][width] u8 device: the same as 0 / 1 bytes
 *   scratch, scratch_bytes  device, 8-byte aligned, at least gs2m_mask_dilate_disk_scratch_bytes(n, width, height) (-1 for
 *                           sizes it refuses); nothing in it outlives the call
 * n = 0 does nothing and returns 0.  Stateless, asynchronous on `stream`, no allocation, no atomics, the same bits on every
 * run; bad arguments return 1 with gs2m_last_error().
 */
int64_t gs2m_mask_dilate_disk_scratch_bytes(int n, int width, int height);
int gs2m_mask_dilate_disk(int n, int width, int height, const uint8_t* const* masks, int radius, uint64_t* out_bits,
                          uint8_t* out_bytes, void* scratch, int64_t scratch_bytes, gs2m_stream stream);

/*
 * The built-in stereo matcher of gs2mesh_amd.stereo_utils.Stereo (stereo_model "SGM"): semi-global matching over four paths
 * on a 9 x 7 census transform.  It stands where the reference runs its stereo network (stereo_utils.py:105-124) and makes no
 * claim to that network's quality; it needs no weights.  Integer arithmetic up to the last step, so the output is defined
 * bit for bit:
 *   1. grey      g = (77 R + 150 G + 29 B + 128) >> 8
 *   2. census    9 wide x 7 high around the pixel without the centre (62 bits): bit = g(neighbour) < g(centre); neighbours
 *                outside the image take the nearest pixel inside
 *   3. cost      left-based pass, d in [0, D): C(y,x,d) = popcount(census_L(y,x) xor census_R(y,x-d)), 62 where x - d < 0
 *   4. paths     r in {right, left, down, up}: L_r = C on the first pixel of a path; after it, with p' the previous pixel and
 *                m = min_k L_r(p',k):  L_r(p,d) = C(p,d) + min(L_r(p',d), L_r(p',d-1) + p1, L_r(p',d+1) + p1, m + p2) - m
 *                (the d-1 / d+1 terms are absent outside [0, D));  S = sum of the four L_r
 *   5. winner    d* = argmin_d S, the lowest d on ties
 *   6. sub-pixel in f32: sm = S(d*-1), sp = S(d*+1), s0 = S(d*), den = sm + sp - 2 s0; if 0 < d* < D-1 and den > 0:
 *                disp = d* + (sm - sp) / (2 den), else disp = d*.  Every pixel gets a value in [0, D-1].
 *   7. disp_rl   the right-based pass (candidate x + d in the left image, cost 62 where x + d >= W): the numbers the reference's
 *                protocol gives, i.e. the left-based matcher on (flip_x(right), flip_x(left)) flipped back.
 *   left_rgb8, right_rgb8   [H][W][3] u8 device (one eye of gs2m_render_views' rgb8)
 *   max_disparity           D: a multiple of 64 in [64, 1024]
 *   p1, p2                  0 < p1 <= p2 <= 190 (a path cost then fits 8 bits)
 *   disp_lr, disp_rl        [H][W] f32 device; either may be NULL (both NULL and no tap: nothing is done)
 *   scratch, scratch_bytes  device, 16-byte aligned, at least gs2m_stereo_sgm_scratch_bytes (-1 for sizes it refuses); the two
 *                           passes share it
 *   tap_cost_lr             NULL, or [H][W][D] u16 device, 16-byte aligned: S of the left-based pass (tests)
 * Asynchronous on `stream`; bad arguments return 1 with gs2m_last_error().
 */
int64_t gs2m_stereo_sgm_scratch_bytes(int width, int height, int max_disparity);
int gs2m_stereo_sgm(const uint8_t* left_rgb8, const uint8_t* right_rgb8, int width, int height, int max_disparity, int p1, int p2,
                    float* disp_lr, float* disp_rl, void* scratch, int64_t scratch_bytes, uint16_t* tap_cost_lr, gs2m_stream stream);

/*
 * The cross-view test between the depth stage and the TSDF: every pixel of every view votes with up to 16 other views
 * ("sources") on whether its depth is a surface they see too.  What depth-map fusion pipelines run before they fuse
 * (COLMAP's geometric consistency, the MVSNet family's filter); the reference has no such stage, so there is nothing to be
 * compatible with and the arithmetic below IS the definition.  In f32, every operation rounded on its own (no FMA, IEEE
 * division), parentheses = order.
 *   valid(view, y, x)  <=>  d = depth[y][x] satisfies d > 0 && d >= min_depth && d < max_depth  (false for NaN; max_depth =
 *                           +inf excludes only the infinities)  and  (mask == NULL || mask[y][x] != 0)
 * For reference view i, pixel (u, v) with valid(i, v, u), d its depth, and each k < max_sources with j = sources[i][k] >= 0,
 * M = pair[i][k]:
 *   x = (((float)u - cx_i) * d) / fx_i,  y = (((float)v - cy_i) * d) / fy_i,  z = d
 *   q_r = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3],  r = 0, 1, 2
 *   !(q_2 > 0): no vote
 *   pu = ((q_0 * fx_j) / q_2 + cx_j) + 0.5f,  pv = ((q_1 * fy_j) / q_2 + cy_j) + 0.5f
 *   !(pu >= 0 && pu < (float)W_j && pv >= 0 && pv < (float)H_j): no vote
 *   iu = (int)floorf(pu), iv = (int)floorf(pv)         (pixel centres at integers: the convention of gs2m_tsdf_integrate)
 *   !valid(j, iv, iu): no vote
 *   diff = depth_j[iv][iu] - q_2,  tol = rel_tol * q_2
 *   fabsf(diff) <= tol: support;  else diff > tol: violation (the source sees past the point: it lies in the source's
 *   observed free space);  else: occluded (the source sees something in front: no evidence either way)
 *   keep = valid(i, v, u) && support >= min_support && violation <= max_violation
 * A pixel that is not valid gets keep = 0 and zero counts.  The same source named twice votes twice.
 *   views                   host array [n_views] of gs2m_depth_view (device pointers); sizes and intrinsics may differ from
 *                           view to view; width and height in 1 .. 65536
 *   max_sources             K, 0 .. 16
 *   sources                 host [n_views][K] int32: index of a source view, -1 = none (anywhere in a row)
 *   pair                    host [n_views][K][12] f32: row-major 3 x 4, reference camera -> source camera (rows of -1 entries
 *                           are not read)
 *   rel_tol                 in (0, 1)
 *   keep, support, violation, occluded
 *                           host arrays [n_views] of [height][width] u8 DEVICE pointers; an array or an entry may be NULL
 *                           (not written); a view none of whose four outputs is asked for costs nothing
 * The host arrays are consumed before the call returns: the descriptors travel as kernel arguments, two reference views per
 * launch.  n_views = 0 does nothing and returns 0.  Stateless, asynchronous on `stream`, no allocation, no atomics, the same
 * bits on every run.  Bad arguments return 1 with gs2m_last_error() and nothing is written: sources[i][k] == i, an index
 * >= n_views or < -1, max_sources > 16, rel_tol outside (0, 1), a view of non-positive (or too large a) size, a NULL depth.
 */
typedef struct gs2m_depth_view { /* host struct, device pointers */
    const float* depth;          /* [height][width] f32 */
    const uint8_t* mask;         /* NULL, or [height][width] u8: 0 = this pixel has no depth */
    int32_t width, height;
    float fx, fy, cx, cy;
} gs2m_depth_view;
int gs2m_depth_consistency(int n_views, const gs2m_depth_view* views, int max_sources, const int32_t* sources, const float* pair,
                           float rel_tol, float min_depth, float max_depth, int min_support, int max_violation,
                           uint8_t* const* keep, uint8_t* const* support, uint8_t* const* violation, uint8_t* const* occluded,
                           gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* nearest neighbours (simple-knn's distCUDA2, the initial scales of 3DGS training)     */
/* ------------------------------------------------------------------------------------ */

/*
 * For every point i of points[P][3] the mean of the three smallest squared distances to the OTHER points
 * (submodules/simple-knn/simple_knn.cu:131-183).  The exact 3-NN, defined bit for bit:
 *   - d(i, j) = (dx * dx + dy * dy) + dz * dz in f32, every operation rounded on its own (no FMA);
 *   - "other" is by index: a duplicate of point i at distance 0 counts;
 *   - a candidate counts only if its d is below the current third best, which starts at FLT_MAX (the reference's
 *     updateKBest, :132-145): a d(i, j) that is NaN or not below FLT_MAX never counts;
 *   - b0 <= b1 <= b2 the three smallest counting d(i, j), j != i, FLT_MAX where fewer than three count;
 *   - out[i] = ((b0 + b1) + b2) / 3.0f  (so P = 3 gives about 1.13e38 and P <= 2 gives +inf, as the reference's arithmetic).
 * Input that is not finite follows from that rule.  A point with a NaN or infinite coordinate has no counting d at all:
 * it gets +inf (not NaN, and this is not an error), and it changes no other point's result.  A point so far away that
 * d(i, j) overflows is a neighbour at "no distance": it contributes FLT_MAX, like a missing one, so a point with only two
 * neighbours in reach gets about 1.13e38 and not +inf.  Subnormal d are kept, never flushed.
 *   points                  [P][3] f32 device
 *   order                   NULL, or [P] int32 device: a permutation of [0, P), position -> index, in which the points are
 *                           walked.  It affects the speed only (sort along a space-filling curve: whole groups of far points
 *                           are then culled by their boxes), never the result.  That it is a permutation is the caller's
 *                           business; an entry outside [0, P) is replaced by its position, so no access leaves the arrays.
 *   scratch, scratch_bytes  device, 16-byte aligned, at least gs2m_knn_scratch_bytes(P); nothing in it outlives the call
 *   out                     [P] f32 device, indexed like `points`
 * P = 0 does nothing and returns 0.  Stateless, asynchronous on `stream`, no allocation; bad arguments return 1 with
 * gs2m_last_error().
 */
int64_t gs2m_knn_scratch_bytes(int P);
int gs2m_knn_mean_dist2(int P, const float* points, const int32_t* order, void* scratch, int64_t scratch_bytes, float* out,
                        gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* mesh evaluation: cross-set nearest neighbour and the DTU surface sampler             */
/* ------------------------------------------------------------------------------------ */

/*
 * For every query i of queries[Q][3] its nearest neighbour among refs[R][3]: the hot path of the reference's geometric
 * metrics (evaluation/DTU/eval_code/eval.py:119-134, evaluation/MobileBrick/eval_code/evaluate.py:46-63), which run it on
 * the host through KD and ball trees.  Exact, defined bit for bit:
 *   - d(i, j) = (dx * dx + dy * dy) + dz * dz in f32, every operation rounded on its own (no FMA);
 *   - selection starts from (+inf, none); candidate j replaces the best when d < best, or when d == best and j is the smaller
 *     index in the caller's numbering ("none" is larger than every index).  A NaN d never replaces.  So exact ties go to the
 *     smallest index and the result is a function of the two point sets alone: not of the orders, not of the launch shape;
 *   - out_d2[i] = the resulting d, out_idx[i] = the resulting j, -1 if none.  R = 0 gives (+inf, -1), so does a query with
 *     a NaN coordinate; a reference with a NaN coordinate is never returned; references farther than f32 can square give
 *     d = +inf with a valid index.
 *   queries, refs           [Q][3], [R][3] f32 device
 *   query_order, ref_order  NULL, or [Q] / [R] int32 device: permutations, position -> index, in which the sets are walked.
 *                           They affect the speed only (sort both along the same space-filling curve: whole groups of far
 *                           references are then culled by their boxes, and the walk starts next to the answer), never the
 *                           result.  An entry outside its range is replaced by its position, so no access leaves the arrays.
 *   scratch, scratch_bytes  device, 16-byte aligned, at least gs2m_nn_scratch_bytes(Q, R) (0 when R = 0: may be NULL);
 *                           nothing in it outlives the call
 *   out_d2                  [Q] f32 device, indexed like `queries`
 *   out_idx                 NULL, or [Q] int32 device
 * Q = 0 does nothing and returns 0.  Stateless, asynchronous on `stream`, no allocation, no atomics, the same bits on every
 * run; bad arguments return 1 with gs2m_last_error().
 */
int64_t gs2m_nn_scratch_bytes(int Q, int R);
int gs2m_nn_dist2(int Q, const float* queries, const int32_t* query_order, int R, const float* refs, const int32_t* ref_order,
                  void* scratch, int64_t scratch_bytes, float* out_d2, int32_t* out_idx, gs2m_stream stream);

/*
 * The DTU evaluation's mesh -> point set (evaluation/DTU/eval_code/eval.py:10-19, 54-71): all vertices, then for every
 * triangle (v0, v1, v2) of non-zero area a regular barycentric grid.  In f64, every operation rounded on its own:
 *   a = v1 - v0, b = v2 - v0;  L1 = sqrt((ax*ax + ay*ay) + az*az), L2 likewise from b;
 *   c = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx),  A = sqrt((cx*cx + cy*cy) + cz*cz);  not A > 0: no samples;
 *   thr = density * sqrt(L1 * L2 / A),  N1 = floor(L1 / thr),  N2 = floor(L2 / thr);
 *   for i = 0 .. N1 (major), j = 0 .. N2 (minor):  c0 = (i + 0.5) / max(N1, 1e-7),  c1 = (j + 0.5) / max(N2, 1e-7),
 *   if c0 + c1 < 1: the next sample is (a * c0 + b * c1) + v0, per component.
 * So N1 = 0 or N2 = 0 gives no sample.  Bit-identical to the reference's sample_single_tri on the grids it was run on
 * (tests/golden/dtu_sample_tri.npz).
 *
 * gs2m_mesh_sample_count writes counts[t] and their exclusive prefix sums offsets[t], synchronises `stream` once and returns
 * the number of samples in *total and these bits in *status:
 *   GS2M_MESH_SAMPLE_CAP     a triangle with (N1 + 1) * (N2 + 1) > 1 048 576 was not sampled (count 0)
 *   GS2M_MESH_SAMPLE_TOTAL   *total > 2^31 - 1: offsets[] wrapped, gs2m_mesh_sample_emit refuses such a total
 *   GS2M_MESH_SAMPLE_INDEX   a triangle names a vertex outside [0, n_vertices); it is never dereferenced (count 0)
 * gs2m_mesh_sample_emit, with the same mesh and density, writes points[n_vertices + total][3]: the vertices, then the
 * samples in triangle order.  No row at or past n_vertices + total is written whatever counts and offsets hold.
 *   vertices                [n_vertices][3] f64 device;  triangles [n_triangles][3] int32 device
 *   counts, offsets         [n_triangles] u32 device
 *   state, state_bytes      device, 8-byte aligned, at least GS2M_MESH_SAMPLE_STATE_BYTES(n_triangles); nothing in it
 *                           outlives the call
 * n_triangles = 0 gives total 0 and emit copies the vertices.  Stateless, no allocation, emit is asynchronous on `stream`;
 * bad arguments return 1 with gs2m_last_error().
 */
#define GS2M_MESH_SAMPLE_CAP 1u
#define GS2M_MESH_SAMPLE_TOTAL 2u
#define GS2M_MESH_SAMPLE_INDEX 4u
#define GS2M_MESH_SAMPLE_STATE_BYTES(n_triangles) (16 + 4 * ((int64_t)(n_triangles) / 4096 + 2))
int gs2m_mesh_sample_count(int64_t n_vertices, const double* vertices, int64_t n_triangles, const int32_t* triangles,
                           double density, uint32_t* counts, uint32_t* offsets, void* state, int64_t state_bytes,
                           gs2m_stream stream, int64_t* total, uint32_t* status);
int gs2m_mesh_sample_emit(int64_t n_vertices, const double* vertices, int64_t n_triangles, const int32_t* triangles,
                          double density, const uint32_t* counts, const uint32_t* offsets, int64_t total, double* points,
                          gs2m_stream stream);

/*
 * The per-view vertex cull of the DTU evaluation (evaluation/DTU/eval_code/evaluate_single_scene.py:63-99): keep[i] = 1 iff
 * point i, in every view, lands outside the image or on that view's mask.  In f32, every operation rounded on its own (no
 * FMA, IEEE division), parentheses = order; (x, y, z) the point, m the view's row-major 3 x 4 projection:
 *   c_k = ((m[k][0] * x + m[k][1] * y) + m[k][2] * z) + m[k][3],  k = 0, 1, 2
 *   u = c_0 / (c_2 + 1e-6f),  v = c_1 / (c_2 + 1e-6f)
 *   gx = (u / (norm_w - 1) - 0.5f) * 2,  gy = (v / (norm_h - 1) - 0.5f) * 2
 *   valid = gx > -1 && gx < 1 && gy > -1 && gy < 1                      (false when anything is NaN)
 *   ix = nearbyint(((gx + 1) / 2) * (mask_width - 1)),  iy = nearbyint(((gy + 1) / 2) * (mask_height - 1))     (ties to even)
 *   s = bit (iy, ix) of the view's bitmap if 0 <= ix < mask_width and 0 <= iy < mask_height (so both finite), else 0
 *   the view passes  <=>  s != 0 || !valid;   keep = every view passes  (n_views = 0 keeps every point)
 * (ix, iy, s) is torch's grid_sampler with mode='nearest', padding_mode='zeros', align_corners=True, which scales by the
 * mask's own size, while the reference normalises by its hard-coded image size: norm_w = 1600, norm_h = 1200 there.  The
 * reference's quirks are part of the statement: a point behind a camera goes through the same formula, and a point outside the
 * open interval passes that view.
 *   points                  [V][3] f32 device
 *   proj                    [n_views][12] f32 device: row-major 3 x 4 (intrinsics @ world-to-camera)
 *   mask_bits               [n_views][mask_height][nw] u64 device, nw = (mask_width + 63) / 64, as gs2m_mask_dilate_disk writes
 *                           them; mask_width, mask_height in 1 .. 2^24
 *   keep                    [V] u8 device: 0 / 1
 * Tolerance against the reference's own lines (`intrinsic @ w2c @ vertices` by torch's matmul, whose summation order is the
 * BLAS's): a keep-bit can differ only where, in some view, the exact (f64) coordinate on the mask's pixel grid lies within
 * tau = 7.6e-5 of a half-integer or of an image bound.  Measured: the f32 sequence above is at most 1.86e-5 of a mask pixel
 * from the f64 value over 1000 points x 3 views of a 130 x 70 mask (tests/test_points_cull.py); tau is 4 x that, the factor
 * for the summation order of the reference's matmul.
 * V = 0 does nothing and returns 0.  Stateless, asynchronous on `stream`, no allocation, no atomics, the result a function of
 * the inputs alone; bad arguments return 1 with gs2m_last_error().
 */
int gs2m_points_cull_views(int V, const float* points, int n_views, const float* proj, const uint64_t* mask_bits, int mask_width,
                           int mask_height, float norm_w, float norm_h, uint8_t* keep, gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* mesh registration: one ICP iteration, and the means of a voxel down-sample           */
/* ------------------------------------------------------------------------------------ */

/*
 * One iteration of point-to-point ICP (Open3D's registration_icp, which the reference runs before it scores MobileBrick and
 * TNT: evaluation/MobileBrick/eval_code/evaluate.py:82-93, evaluation/TNT/eval_code/python_toolbox/evaluation/registration.py)
 * between source[N][3] and target[R][3], both f64: the pairs of the current transform and the moments of the kept ones.
 *
 * gs2m_icp_prepare, once per registration, builds the search structure of the target in `scratch`: the records, boxes and
 * super-boxes that gs2m_nn_dist2 builds per call, of the f32 points f32(target - origin), the subtraction in f64.  It stays
 * valid for every later gs2m_icp_step with the same target, origin and scratch, whatever their N.
 *
 * gs2m_icp_step, in f64 unless said otherwise, every operation rounded on its own (no FMA), parentheses = order; T the
 * row-major 4 x 4 `transform` (its last row is not read), o the origin, s = source[i]:
 *   p_k  = ((T[k][0] * s_x + T[k][1] * s_y) + T[k][2] * s_z) + T[k][3],  k = 0, 1, 2
 *   j    = the nearest neighbour of f32(p - o) among f32(target - o) by the rule of gs2m_nn_dist2 (f32 distance, exact, ties
 *          to the smallest index, a NaN distance never selected; -1 if none: R = 0, or p has a NaN coordinate)
 *   q    = target[j],  d2 = ((p_x - q_x)^2 + (p_y - q_y)^2) + (p_z - q_z)^2
 *   kept <=> j >= 0 and d2 < max_dist * max_dist        (strict, as Open3D's hybrid search is remembered to be; false on NaN)
 *   p' = p - o,  q' = q - o
 * and over the kept pairs the 18 eight-byte slots of `sums`:
 *   [0] n, the number of kept pairs, as int64;  [1] sum d2;  [2..4] sum p';  [5..7] sum q';
 *   [8 + 3 a + b] sum p'_a * q'_b;  [17] sum ((p'_x^2 + p'_y^2) + p'_z^2).
 * Every f64 sum is added in one fixed order, without atomics: thread t of workgroup b adds the kept pairs among
 * i = 1024 b + t + 256 k, k = 0 .. 3, in that order from +0; the 64 lanes of a wave by six rounds v = v + v[lane ^ m],
 * m = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; the workgroups' partials t, t + 256, ... by thread t of one
 * last workgroup, reduced the same way.  So the sums are a function of (source, T, target, o, max_dist) alone: not of the
 * orders, not of the run.  The shift by o keeps the raw moments conditioned like the centred ones when o lies in the scene.
 *   source, target          [N][3], [R][3] f64 device;  the same `target` that was prepared
 *   query_order, ref_order  NULL, or [N] / [R] int32 device: as in gs2m_nn_dist2, the speed only
 *   transform, origin       HOST, 16 and 3 f64, read before the call returns
 *   max_dist                positive and finite, or the call is refused
 *   scratch, scratch_bytes  device, 16-byte aligned, at least gs2m_icp_scratch_bytes(N, R); prepare needs
 *                           gs2m_icp_scratch_bytes(0, R) of it.  Size it once for the largest N (gs2m_scratch_refused's contract)
 *   sums                    device, 8-byte aligned, 18 * 8 bytes
 *   out_idx, out_d2         NULL, or [N] int32 / [N] f64 device: j and d2 of every source point (d2 = +inf where j = -1)
 * N = 0 writes zero sums; R = 0 gives n = 0 (prepare does nothing then).  Stateless apart from the scratch, asynchronous on
 * `stream` with no host wait, no allocation; bad arguments return 1 with gs2m_last_error().
 */
int64_t gs2m_icp_scratch_bytes(int N, int R);
int gs2m_icp_prepare(int R, const double* target, const double* origin, const int32_t* ref_order, void* scratch,
                     int64_t scratch_bytes, gs2m_stream stream);
int gs2m_icp_step(int N, const double* source, const int32_t* query_order, const double* transform, int R, const double* target,
                  const double* origin, double max_dist, void* scratch, int64_t scratch_bytes, void* sums, int32_t* out_idx,
                  double* out_d2, gs2m_stream stream);

/*
 * The accumulation of Open3D's PointCloud::VoxelDownSample on points already grouped by voxel: segment s is
 * order[heads[s] .. heads[s + 1]) (the last one ends at N); means[s] = (((0 + x_0) + x_1) + ...) / count per axis in f64, the
 * rows added in the order `order` lists them.  With `order` a stable sort by voxel key that is ascending original index, the
 * order in which Open3D's AccumulatedPoint adds them.  An empty segment gives NaN (0 / 0).
 *   points                  [N][3] f64 device;  order [N] int32 device;  heads [S] int32 device, ascending, heads[0] = 0
 *   means                   [S][3] f64 device
 * An entry of `order` outside [0, N) or a head outside [0, N] is clamped, so no access leaves the arrays.  S = 0 does nothing.
 * Stateless, asynchronous on `stream`, no allocation, no atomics; bad arguments return 1 with gs2m_last_error().
 */
int gs2m_voxel_mean(int N, const double* points, const int32_t* order, int S, const int32_t* heads, double* means,
                    gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* photometric loss of 3DGS training (L1 + D-SSIM, GS/utils/loss_utils.py, train.py:89-90) */
/* ------------------------------------------------------------------------------------ */

/*
 * loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean(m)),  m the SSIM map of x = image and y = target: 11 x 11 Gaussian
 * window (sigma 1.5, normalised), zero padding, per plane, C1 = 0.01^2, C2 = 0.03^2.  N = planes * height * width.
 * Defined operation by operation in f32, every operation rounded on its own (no FMA, IEEE division), parentheses = order:
 *   - w[k], k = 0 .. 10: exp(-(k - 5)^2 / 4.5) normalised by the sum in index order, in double on the host, cast to f32 last;
 *   - F(q) = V(H(q)), H(q)(r, c) = sum_k w[k] * q(r, c + k - 5), V(h)(r, c) = sum_k w[k] * h(r + k - 5, c); every sum is
 *     acc = 0, then acc = acc + w[k] * term for k = 0 .. 10; q and H(q) are 0 outside the image (the 2-D window is the outer
 *     product of w, so this is the reference's filter at 22 taps);
 *   - mu1 = F(x), mu2 = F(y), exx = F(x * x), eyy = F(y * y), exy = F(x * y);  m11 = mu1 * mu1, m22 = mu2 * mu2,
 *     m12 = mu1 * mu2, s1 = exx - m11, s2 = eyy - m22, s12 = exy - m12;
 *   - A = (m11 + m22) + C1, B = (s1 + s2) + C2, C = 2 * m12 + C1, D = 2 * s12 + C2, AB = A * B, m = (C * D) / AB
 *     (identical images give m = 1 exactly);
 *   - partials[0] = dm/dmu1 = 2 * ((((mu2 * D) / AB - (mu2 * C) / AB) - (mu1 * m) / A) + (mu1 * m) / B),
 *     partials[1] = dm/dsigma1^2 = -(m / B),  partials[2] = dm/dsigma12 = (2 * C) / AB;
 *   - out = { (ka * S1 + f32(lambda)) - kb * Sm,  S1 * f32(1 / N),  Sm * f32(1 / N) } with S1 = sum |x - y|, Sm = sum m,
 *     ka = f32((1 - lambda) / N), kb = f32(lambda / N), the quotients in double.  The sums use no atomics and a fixed order
 *     (per thread, a tree per 32 x 16 tile, then one workgroup over the tiles): the same bits on every run, and the longest
 *     addition chain is 2 + 8 + ceil(tiles / 1024) + 10, tiles = planes * ceil(height / 16) * ceil(width / 32);
 *   - backward: gl = grad_loss[0], g = gl * (-kb), l = gl * ka,
 *     grad_image = ((F(g * partials[0]) + (2 * x) * F(g * partials[1])) + y * F(g * partials[2])) + l * sign(x - y),
 *     sign = (d > 0) - (d < 0), so 0 where x = y as torch's abs has it.  No gradient is computed for the target.
 * Measured against the fp64 evaluation of the reference's formulas on the four inputs of tests/test_photo_loss_statement.py
 * (N from 84 to 23 040; the f32 torch path on the same inputs in brackets): SSIM map 1.9e-6 on noise [5.1e-6], up to 3.7e-4
 * on smooth near-identical images, where sigma^2 cancels [9.2e-4]; loss at most 8.4e-7 [2.7e-7]; the gradient scales with
 * 1 / N, and N * |error| is at most 2.4e-4 [5.8e-4] (entries N * |g| up to 8.4).  Stated tolerance against fp64: loss 1e-6 plus
 * 2^-24 per addition of the chain, map 4e-4, gradient 3e-4 / N.  Stated tolerance against loss_fn evaluated in f32, which errs
 * too (the two measured errors added; for the loss also the chain's 21 * 2^-24): loss 2.5e-6, gradient 1e-3 / N.
 *   planes, height, width   planes * height * width = 0 does nothing and returns 0; at most 2^23 tiles
 *   image, target           [planes][height][width] f32 device
 *   lambda_dssim            the reference's 0.2
 *   scratch, scratch_bytes  device, 16-byte aligned, at least gs2m_photo_loss_scratch_bytes (-1 for sizes it refuses);
 *                           nothing in it outlives the call
 *   out                     [3] f32 device: loss, mean |x - y|, mean SSIM
 *   partials                NULL (no backward will follow), or [3][planes][height][width] f32 device
 *   tap_map                 NULL, or [planes][height][width] f32 device: m (tests)
 *   grad_loss               [1] f32 device: autograd's incoming gradient, never read on the host
 *   grad_image              [planes][height][width] f32 device, written in full
 * Stateless, asynchronous on `stream`, no allocation; a NULL pointer, a negative size and a short or misaligned scratch
 * return 1 with a gs2m_last_error() that names the argument.
 */
int64_t gs2m_photo_loss_scratch_bytes(int planes, int height, int width);
int gs2m_photo_loss_forward(int planes, int height, int width, const float* image, const float* target, float lambda_dssim,
                            void* scratch, int64_t scratch_bytes, float* out, float* partials, float* tap_map, gs2m_stream stream);
int gs2m_photo_loss_backward(int planes, int height, int width, const float* image, const float* target, const float* partials,
                             float lambda_dssim, const float* grad_loss, float* grad_image, gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* training update: Adam step over several tensors, densification statistics            */
/* ------------------------------------------------------------------------------------ */

/*
 * One Adam step (Kingma & Ba; the update torch.optim.Adam makes with amsgrad, weight decay and maximize off) of up to 8
 * "segments" in ONE kernel launch.  A segment is a contiguous f32 tensor with its gradient, its two moments and its own
 * scalars; t = step is the number of the step being taken (1 for the first).  Defined operation by operation in f32, every
 * operation rounded on its own (no FMA), IEEE division and square root, subnormals kept (never flushed), parentheses = order:
 *   - on the host, in double, cast to f32 last:  ss = f32(lr / (1 - beta1^t)),  bs = f32(sqrt(1 - beta2^t)),
 *     omb1 = f32(1 - beta1),  b2 = f32(beta2),  omb2 = f32(1 - beta2),  e = f32(eps);  beta^t is pow(beta, (double)t);
 *   - m' = m + omb1 * (g - m)
 *   - v' = b2 * v + (omb2 * g) * g
 *   - p' = p - ss * (m' / (sqrt(v') / bs + e))
 * with p = param, g = grad, m = exp_avg, v = exp_avg_sq, updated in place.  One lane owns each element and nothing is
 * accumulated across elements: the same bits on every run.  Special values follow from the operations: g = 0 with m = v = 0
 * gives 0 / e = 0 and leaves p; |g| = 1e-20 gives the subnormal (omb2 * g) * g = 1e-43 (the product g * g is never formed); for
 * the same reason |g| = 1e20, whose square overflows, gives the finite 1e37 and an ordinary step; from |g| of about 5.8e20 on
 * (at beta2 = 0.999) v' overflows to +inf, the quotient is 0 and p stays, on that step and on those after it; a NaN or
 * infinite g makes p NaN.
 * tests/adam_statement.py restates this in numpy and the kernel agrees with it bit for bit on both back-ends.
 *
 * Distance of this form from the two usual evaluations, measured on the CPU with the numpy statement (200 000 elements,
 * p ~ N(0, 1), gradients N(0, 1) * 10^U(-8, 0) with a third of them exactly 0 every seventh step, from m = v = 0; three seeds
 * times (lr, eps, betas) = (0.0025, 1e-15, 0.9 / 0.999), (0.05, ...), (0.00016, ...), (0.001, 1e-8, 0.8 / 0.99)).  The unit is
 * u(T) = ulp(p) + T * lr * 2^-23 for T steps: the rounding of p plus the rounding of T steps of size about lr (p may have been
 * up to T * lr larger in magnitude on the way, with the larger ulp that goes with it).  Largest |p - yardstick| / u(T):
 *   against Adam evaluated in double (torch's formulas) from the same f32 state, one step, t = 1 .. 50:      2.13
 *   against torch.optim.Adam(foreach=False) on CPU tensors, first step:                                     1.20
 *   50 carried steps against Adam carried in double:                                                        11.8
 *   50 carried steps against torch.optim.Adam(foreach=False) carried in f32:                                2.40
 * Stated tolerances, the measurements x 4 for inputs not tried, rounded up: GS2M_ADAM_TOL_FP64_STEP = 9, _TORCH_STEP = 5 (in
 * u(1)), GS2M_ADAM_TOL_FP64_50 = 48, _TORCH_50 = 10 (in u(50)).  The form is not bit-equal to torch (no single-rounding
 * formula is: torch's own CPU and GPU paths differ from each other).
 *
 * Row-sparse mode (row_visible != NULL): every segment is [rows][row_width]; element e belongs to row e / row_width and
 * is updated only where row_visible[row] > 0 (the rasteriser's radii serve as the mask).  Elements of the other rows are
 * neither read nor written: p, m and v keep their bits and their gradient entries may hold anything.  The arithmetic and the
 * scalars are the same as above: the bias correction is that of `step`, not of a per-row count, and the moments of an unseen
 * row do not decay.  With every row visible the call equals the dense call bit for bit.
 *
 *   n_segments, segments    1 .. 8; a HOST array, read before the call returns.  Segments with count == 0 are skipped; with
 *                           every count 0 nothing is launched
 *   param, grad, exp_avg,   device, count f32 each.  16-byte aligned pointers are moved 16 bytes per lane; others work,
 *   exp_avg_sq              4 bytes at a time.  No two ranges of the call may overlap (row_visible included)
 *   row_width               >= 1; used in row-sparse mode, where count must be rows * row_width
 *   step                    >= 1;  betas in [0, 1)
 *   row_visible, rows       NULL, or [rows] int32 device
 * Stateless, asynchronous on `stream`, no allocation, no copy.  n_segments outside 1 .. 8, a NULL pointer with count > 0,
 * a negative count, row_width < 1, step < 1, a beta outside [0, 1), a count that is not rows * row_width, overlapping ranges
 * and a call of more than 2^31 - 1 workgroups of 1024 elements return 1 with gs2m_last_error(); nothing is written then.
 */
#define GS2M_ADAM_MAX_SEGMENTS 8
#define GS2M_ADAM_TOL_FP64_STEP 9.0
#define GS2M_ADAM_TOL_TORCH_STEP 5.0
#define GS2M_ADAM_TOL_FP64_50 48.0
#define GS2M_ADAM_TOL_TORCH_50 10.0
typedef struct gs2m_adam_segment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
    int64_t step;
    int32_t row_width;
    int32_t reserved; /* 0 */
    double lr, beta1, beta2, eps;
} gs2m_adam_segment;
int gs2m_adam_step(int n_segments, const gs2m_adam_segment* segments, const int32_t* row_visible, int64_t rows,
                   gs2m_stream stream);

/*
 * The densification statistics of one training iteration (GS/train.py:113-115, gaussian_model.py:405-407), one Gaussian per
 * lane.  Where radii[i] > 0, every operation one f32 operation rounded on its own, IEEE square root:
 *   r = (float)radii[i];  max_radii2D[i] = r > max_radii2D[i] ? r : max_radii2D[i]
 *   n = sqrt(gx * gx + gy * gy), (gx, gy) = viewspace_grad[i][0 .. 1];  grad_accum[i] = grad_accum[i] + n;
 *   denom[i] = denom[i] + 1
 * Rows with radii[i] <= 0 are neither read (beyond radii) nor written.  denom and max_radii2D equal the torch ops of the
 * reference's loop exactly.  n carries three roundings and torch.norm over the two columns at least one: they differ by at
 * most 2 ulp(n), and after the addition to grad_accum >= n by at most 2 ulp(n) + 1 ulp(grad_accum) <= 3 ulp(grad_accum) =
 * GS2M_DENSIFY_ACCUM_TOL_ULP per update.  Measured on the CPU over 100 000 rows of N(0, 1) * 10^U(-8, 0): n 1 ulp, grad_accum 2.
 *   P                       0 does nothing and returns 0
 *   radii                   [P] int32 device
 *   viewspace_grad          [P][3] f32 device
 *   max_radii2D, grad_accum, denom   [P] f32 device, updated in place
 * Stateless, asynchronous on `stream`; a negative P or a NULL pointer returns 1 with gs2m_last_error().
 */
#define GS2M_DENSIFY_ACCUM_TOL_ULP 3
int gs2m_densify_stats(int P, const int32_t* radii, const float* viewspace_grad, float* max_radii2D, float* grad_accum,
                       float* denom, gs2m_stream stream);

/* ------------------------------------------------------------------------------------ */
/* PNG encoder (the Renderer's left.png / right.png)               */
/* ------------------------------------------------------------------------------------ */

/*
 * Replaces the PIL / cv2 PNG writes of Renderer.render_image_pair (gs2mesh_utils/renderer_utils.py:389-390): the files are
 * made on the device and only the compressed bytes cross to the host.  The stream (gs2mesh_amd/csrc/png_encode.hip):
 * 8-bit RGB, IHDR / one IDAT / IEND; filter `filter` on every row; the filtered scanlines cut into segments of
 * rows_per_segment rows, each one deflate block with a dynamic Huffman code of its own (literals only, lengths <= 15)
 * followed by an empty stored block, or stored blocks when that is not smaller.  Output bytes depend only on the pixels,
 * rows_per_segment and filter (the same on every device and batch size).
 *   gs2m_png_max_bytes  upper bound of one file (every segment stored); -1 for sizes it cannot encode.
 *   gs2m_png_encode     rgb8: device [n, H, W, 3] u8 (image k at rgb8 + k*image_stride bytes); out: device [n, out_stride]
 *                       u8 with out_stride >= gs2m_png_max_bytes; out_bytes: device [n] int64, file k = out[k, :out_bytes[k]].
 *                       filter: 0 (none) or 4 (Paeth, default); rows_per_segment: >= 1 (default 16).
 *                       Stream-ordered, no host synchronisation; the handle's grow-only scratch is allocated on the
 *                       first call at a size (that call synchronises).
 */
typedef struct gs2m_png gs2m_png;
int gs2m_png_create(gs2m_png** out, int device);
int gs2m_png_destroy(gs2m_png* p);
int64_t gs2m_png_max_bytes(int width, int height, int rows_per_segment);
int gs2m_png_encode(gs2m_png* p, int n, int width, int height, const uint8_t* rgb8, int64_t image_stride, uint8_t* out,
                    int64_t out_stride, int64_t* out_bytes, int filter, int rows_per_segment, gs2m_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* GS2MESH_AMD_H */
