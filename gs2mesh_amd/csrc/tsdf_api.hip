// tsdf_api.hip -- C ABI of the TSDF half (include/gs2mesh_amd.h).  Host code; kernels in
// tsdf_kernels.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/gs2mesh_amd.h"
#include "device_memory.h"
#include "tsdf_common.h"
#include "tsdf_internal.h"

struct gs2m_tsdf {
    int device = 0;
    double voxel_length = 0, sdf_trunc = 0, unit_length = 0;
    int color_type = 1, resolution = 16, stride = 4;
    TsdfVolume V;           // what the kernels get, by value: the pointers of `vol` below and the sizes, filled once at creation
    struct {                // owners of V's arrays (sizes: tsdf_common.h)
        DeviceBuffer<float> tsdf, weight;
        DeviceBuffer<unsigned> rgb, stamp, touched, counters;
        DeviceBuffer<int> block_keys, hash_vals;
        DeviceBuffer<unsigned char> halo;
        DeviceBuffer<unsigned long long> hash_keys, fmask, totals;
    } vol;
    unsigned frame_id = 0;  // monotonic, never reset (stamps of old frames can never alias)
    PinnedBuffer<unsigned> h_counters;           // [4]
    PinnedBuffer<unsigned long long> h_totals;   // [1]
    int n_cu = 256;
    DeviceBuffer<unsigned char> d_mc;            // marching-cubes case table (McDevTables, generated at create)
    const McDevTables* mc() const { return reinterpret_cast<const McDevTables*>(d_mc.get()); }
    DeviceBuffer<unsigned> d_blk_tris;           // [max_blocks] per-block triangle counts / offsets
    DeviceBuffer<unsigned long long> d_ntri;     // [1]
    // the last mesh gs2m_tsdf_extract_mesh produced, welded, on the device (read with gs2m_tsdf_mesh_copy); grow-only
    DeviceBuffer<double> mesh_v, mesh_c;   // [mesh_nv][3]
    DeviceBuffer<int> mesh_e;              // [mesh_nv][4]
    DeviceBuffer<int> mesh_tri;            // [mesh_nt][3]
    int64_t mesh_nv = 0, mesh_nt = 0;
    ScratchArena mesh_scratch;             // the extraction's temporaries (soup, weld table, scan)
    int timing = 0;
    EventPool events;                      // weight = frames the timed launch covered (a batch counts as that many launches)
    DeviceBuffer<TsdfBatchFrame> d_bframes;   // [GS2M_TSDF_MAX_BATCH] frame descriptors of the batch in flight
    DeviceBuffer<float> d_tiles;              // the batch's max-depth map (tsdf_common.h): grow-only, GS2M_TSDF_MAX_BATCH frames of the largest image seen
    // pinned staging ring for the descriptors (a pageable source would make the "async" copy wait for the stream)
    static const int kRing = 8;
    PinnedBuffer<TsdfBatchFrame> h_bframes;   // [kRing][GS2M_TSDF_MAX_BATCH]
    hipEvent_t ring_done[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned ring_next = 0;
    ~gs2m_tsdf() {
        for (auto e : ring_done)
            if (e) (void)hipEventDestroy(e);
    }
};

// General 4x4 inverse (cofactors), double.  The reference hands Open3D world->camera and
// Open3D inverts it again (PointCloudFactory.cpp: camera_pose = extrinsic.inverse()).
static bool invert4x4(const double* m, double* inv) {
    double a[16];
    a[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    a[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    a[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    a[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    a[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    a[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    a[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    a[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    a[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    a[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    a[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    a[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    a[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    a[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    a[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    a[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    double det = m[0] * a[0] + m[1] * a[4] + m[2] * a[8] + m[3] * a[12];
    if (det == 0) return false;
    det = 1.0 / det;
    for (int i = 0; i < 16; i++) inv[i] = a[i] * det;
    return true;
}

// `whole_pool`: at creation (fresh device memory is not zero); later resets only clear the slots that were handed out
static int zero_state(gs2m_tsdf* t, hipStream_t st, bool whole_pool, long long keep_first = -1) {
    TsdfVolume& V = t->V;
    if (whole_pool) {
        GS2M_HIPCHK(hipMemsetAsync(V.tsdf, 0, sizeof(float) * (size_t)V.max_blocks * GS2M_TSDF_VOX, st));
        GS2M_HIPCHK(hipMemsetAsync(V.weight, 0, sizeof(float) * (size_t)V.max_blocks * GS2M_TSDF_VOX, st));
        if (V.rgb) GS2M_HIPCHK(hipMemsetAsync(V.rgb, 0, sizeof(unsigned) * 3 * (size_t)V.max_blocks * GS2M_TSDF_VOX, st));
        GS2M_HIPCHK(hipMemsetAsync(V.halo, 0, (size_t)V.max_blocks, st));
    } else if (keep_first < 0) {
        gs2m_launch_tsdf_clear_used(st, V);   // reads counters[0] on the device: no host sync
    } else {
        gs2m_launch_tsdf_clear_from(st, V, (unsigned)keep_first);   // gs2m_tsdf_replace: slots [0, keep_first) are overwritten next
    }
    GS2M_HIPCHK(hipMemsetAsync(V.hash_keys, 0xff, sizeof(unsigned long long) * (size_t)V.hash_cap, st));
    GS2M_HIPCHK(hipMemsetAsync(V.hash_vals, 0xff, sizeof(int) * (size_t)V.hash_cap, st));
    GS2M_HIPCHK(hipMemsetAsync(V.stamp, 0, sizeof(unsigned) * (size_t)V.hash_cap, st));
    GS2M_HIPCHK(hipMemsetAsync(V.fmask, 0, sizeof(unsigned long long) * (size_t)V.hash_cap, st));
    GS2M_HIPCHK(hipMemsetAsync(V.counters, 0, sizeof(unsigned) * 4, st));
    GS2M_HIPCHK(hipMemsetAsync(V.totals, 0, sizeof(unsigned long long), st));
    return 0;
}

// allocates and clears the volume of a new handle, whose scalar fields are set; on failure the caller deletes the handle
static int init_volume(gs2m_tsdf* t, int64_t max_blocks) {
    memset(&t->V, 0, sizeof(t->V));
    TsdfVolume& V = t->V;
    V.max_blocks = (unsigned)max_blocks;
    unsigned cap = 1024;
    while ((uint64_t)cap < 2ull * (uint64_t)max_blocks) cap <<= 1;
    V.hash_cap = cap;
    V.has_color = t->color_type == GS2M_TSDF_COLOR_RGB8;
    const size_t nvox = (size_t)max_blocks * GS2M_TSDF_VOX, nb = (size_t)max_blocks;
    auto& o = t->vol;
    if (o.tsdf.reserve_exact(nvox) || o.weight.reserve_exact(nvox) || (V.has_color && o.rgb.reserve_exact(3 * nvox)) ||
        o.block_keys.reserve_exact(3 * nb) || o.halo.reserve_exact(nb) || o.hash_keys.reserve_exact(cap) ||
        o.hash_vals.reserve_exact(cap) || o.stamp.reserve_exact(cap) || o.touched.reserve_exact(cap) || o.fmask.reserve_exact(cap) ||
        t->d_bframes.reserve_exact(GS2M_TSDF_MAX_BATCH) || t->h_bframes.reserve(GS2M_TSDF_MAX_BATCH * gs2m_tsdf::kRing) ||
        o.counters.reserve_exact(4) || o.totals.reserve_exact(1) || t->d_mc.reserve_exact(gs2m_mc_tables_bytes()) ||
        t->d_blk_tris.reserve_exact(nb) || t->d_ntri.reserve_exact(1) || t->h_counters.reserve(4) || t->h_totals.reserve(1)) {
        gs2m_set_error("gs2m_tsdf_create: out of device memory for %lld blocks (%.1f MiB)", (long long)max_blocks,
                       (double)nvox * 20.0 / 1048576.0);
        return 1;
    }
    V.tsdf = o.tsdf.get();
    V.weight = o.weight.get();
    V.rgb = o.rgb.get();   // null without colour
    V.block_keys = o.block_keys.get();
    V.halo = o.halo.get();
    V.hash_keys = o.hash_keys.get();
    V.hash_vals = o.hash_vals.get();
    V.stamp = o.stamp.get();
    V.touched = o.touched.get();
    V.fmask = o.fmask.get();
    V.counters = o.counters.get();
    V.totals = o.totals.get();
    std::vector<unsigned char> tab(gs2m_mc_tables_bytes());
    if (!gs2m_mc_tables_fill(tab.data()) ||
        hipMemcpy(t->d_mc.get(), tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
        gs2m_set_error("gs2m_tsdf_create: marching-cubes table generation failed");
        return 1;
    }
    if (zero_state(t, (hipStream_t)0, true)) return 1;
    GS2M_HIPCHK(hipStreamSynchronize((hipStream_t)0));
    return 0;
}

extern "C" int gs2m_tsdf_create(gs2m_tsdf** out, double voxel_length, double sdf_trunc, int color_type,
                                int volume_unit_resolution, int depth_sampling_stride, int64_t max_blocks,
                                int device) {
    if (!out) {
        gs2m_set_error("gs2m_tsdf_create: out is NULL");
        return 1;
    }
    if (volume_unit_resolution != GS2M_TSDF_RES) {
        gs2m_set_error("volume_unit_resolution %d not supported (kernels are specialised for 16, Open3D's default)",
                       volume_unit_resolution);
        return 1;
    }
    if (!(voxel_length > 0) || !(sdf_trunc > 0) || depth_sampling_stride < 1 || max_blocks < 1 ||
        max_blocks > (1ll << 30) || (color_type != GS2M_TSDF_COLOR_NONE && color_type != GS2M_TSDF_COLOR_RGB8)) {
        gs2m_set_error("gs2m_tsdf_create: bad argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(device));
    gs2m_tsdf* t = new gs2m_tsdf();
    t->device = device;
    t->voxel_length = voxel_length;
    t->sdf_trunc = sdf_trunc;
    t->unit_length = voxel_length * volume_unit_resolution;  // ScalableTSDFVolume ctor
    t->color_type = color_type;
    t->stride = depth_sampling_stride;
    if (init_volume(t, max_blocks)) {
        delete t;
        return 1;
    }
    *out = t;
    return 0;
}

extern "C" int gs2m_tsdf_destroy(gs2m_tsdf* t) {
    delete t;   // every buffer and event is a member
    return 0;
}

extern "C" int gs2m_tsdf_reset(gs2m_tsdf* t, gs2m_stream stream) {
    if (!t) {
        gs2m_set_error("null handle");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    return zero_state(t, (hipStream_t)stream, false);
}

// per-frame uniforms (intrinsics, pose, truncation constants) of one integrate call
static int fill_frame(gs2m_tsdf* t, TsdfFrame& f, int width, int height, double fx, double fy, double cx, double cy,
                      const double* extrinsic_w2c, double depth_scale, double depth_trunc, double min_depth, bool has_mask) {
    memset(&f, 0, sizeof(f));
    double pose[16];
    if (!invert4x4(extrinsic_w2c, pose)) {
        gs2m_set_error("gs2m_tsdf_integrate: singular extrinsic");
        return 1;
    }
    for (int i = 0; i < 12; ++i) {
        f.pose[i] = pose[i];
        f.E[i] = (float)extrinsic_w2c[i];
    }
    f.fx = fx;
    f.fy = fy;
    f.cx = cx;
    f.cy = cy;
    f.unit_length = t->unit_length;
    f.sdf_trunc = t->sdf_trunc;
    f.depth_trunc = depth_trunc;
    f.fx_f = (float)fx;
    f.fy_f = (float)fy;
    f.cx_f = (float)cx;
    f.cy_f = (float)cy;
    f.fx_inv_f = 1.0f / (float)fx;
    f.fy_inv_f = 1.0f / (float)fy;
    f.voxel_length_f = (float)t->voxel_length;
    f.half_voxel_length_f = f.voxel_length_f * 0.5f;
    f.sdf_trunc_f = (float)t->sdf_trunc;
    f.sdf_trunc_inv_f = 1.0f / f.sdf_trunc_f;
    f.Es02 = f.E[2] * f.voxel_length_f;
    f.Es12 = f.E[6] * f.voxel_length_f;
    f.Es22 = f.E[10] * f.voxel_length_f;
    f.safe_w = width - 0.0001f;
    f.safe_h = height - 0.0001f;
    f.depth_scale_f = (float)depth_scale;
    f.min_depth_f = (float)min_depth;
    // Image::ConvertDepthToFloatImage compares the float depth with the double threshold; the same decision in fp32:
    f.depth_trunc_up_f = (float)depth_trunc;
    if ((double)f.depth_trunc_up_f < depth_trunc) f.depth_trunc_up_f = nextafterf(f.depth_trunc_up_f, INFINITY);
    f.W = width;
    f.H = height;
    f.stride = t->stride;
    f.nx = (width + t->stride - 1) / t->stride;
    f.ny = (height + t->stride - 1) / t->stride;
    f.frame_id = ++t->frame_id;
    f.use_mask = has_mask;
    f.use_min = min_depth > 0;
    return 0;
}

// size and intrinsics as both integrate entry points require them; `max_side`: the largest width / height the caller's kernels
// can address (0 = no limit of their own), named by `limit_note`
static int check_frame_geometry(const char* who, int width, int height, double fx, double fy, double depth_scale, int max_side,
                                const char* limit_note) {
    if (width <= 0 || height <= 0 || (max_side && (width > max_side || height > max_side)) || !(fx != 0) || !(fy != 0) ||
        !(depth_scale != 0)) {
        gs2m_set_error("%s: bad intrinsics / size%s", who, limit_note);
        return 1;
    }
    return 0;
}

extern "C" int gs2m_tsdf_integrate(gs2m_tsdf* t, const float* depth, const uint8_t* color, const uint8_t* mask,
                                   int width, int height, double fx, double fy, double cx, double cy,
                                   const double* extrinsic_w2c, double depth_scale, double depth_trunc,
                                   double min_depth, gs2m_stream stream) {
    if (!t || !depth || !extrinsic_w2c) {
        gs2m_set_error("gs2m_tsdf_integrate: NULL argument");
        return 1;
    }
    if (t->V.has_color && !color) {
        // Open3D: "[ScalableTSDFVolume::Integrate] Unsupported image format."
        gs2m_set_error("[ScalableTSDFVolume::Integrate] Unsupported image format.");
        return 1;
    }
    if (check_frame_geometry("gs2m_tsdf_integrate", width, height, fx, fy, depth_scale, 0, "")) return 1;
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    TsdfFrame f;
    if (fill_frame(t, f, width, height, fx, fy, cx, cy, extrinsic_w2c, depth_scale, depth_trunc, min_depth, mask != nullptr))
        return 1;
    GS2M_HIPCHK(hipMemsetAsync(t->V.counters + 1, 0, sizeof(unsigned), st));  // touched_count = 0
    {
        StageTimer tm(t->events, t->timing != 0, st, 0, "gs2m:tsdf_touch");
        gs2m_launch_tsdf_touch(st, t->V, f, depth, mask);
    }
    {
        // persistent grid: enough workgroups to fill the chip; each loops over the touched list
        StageTimer tm(t->events, t->timing != 0, st, 1, "gs2m:tsdf_integrate");
        gs2m_launch_tsdf_integrate(st, t->n_cu * 7, t->V, f, depth, color, mask);
    }
    return 0;
}

extern "C" int gs2m_tsdf_integrate_batch(gs2m_tsdf* t, int n_frames, const float* const* depth, const uint8_t* const* color,
                                         const uint8_t* const* mask, int width, int height, double fx, double fy, double cx,
                                         double cy, const double* extrinsics_w2c, double depth_scale, double depth_trunc,
                                         double min_depth, gs2m_stream stream) {
    if (!t || n_frames < 0 || (n_frames > 0 && (!depth || !extrinsics_w2c))) {
        gs2m_set_error("gs2m_tsdf_integrate_batch: NULL argument");
        return 1;
    }
    if (t->V.has_color && n_frames > 0 && !color) {
        gs2m_set_error("[ScalableTSDFVolume::Integrate] Unsupported image format.");
        return 1;
    }
    if (n_frames > 0 && check_frame_geometry("gs2m_tsdf_integrate_batch", width, height, fx, fy, depth_scale, 65535,
                                             " (the sweep packs pixel coordinates in 16 bits: <= 65535)"))
        return 1;
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    // sized for a full batch on the first use of an image size, so that a later, longer sweep of such images allocates nothing
    if (n_frames > 0 && t->d_tiles.reserve_exact((size_t)GS2M_TSDF_MAX_BATCH * GS2M_TSDF_TILES(width) * GS2M_TSDF_TILES(height))) return 1;
    for (int f0 = 0; f0 < n_frames; f0 += GS2M_TSDF_MAX_BATCH) {
        const int nf = n_frames - f0 < GS2M_TSDF_MAX_BATCH ? n_frames - f0 : GS2M_TSDF_MAX_BATCH;
        // next slot of the pinned staging ring; its previous copy (kRing batches ago) has long completed
        const unsigned slot = t->ring_next++ % gs2m_tsdf::kRing;
        if (t->ring_done[slot]) GS2M_HIPCHK(hipEventSynchronize(t->ring_done[slot]));
        else GS2M_HIPCHK(hipEventCreateWithFlags(&t->ring_done[slot], hipEventDisableTiming));
        TsdfBatchFrame* hb = t->h_bframes.get() + (size_t)slot * GS2M_TSDF_MAX_BATCH;
        for (int k = 0; k < nf; ++k) {
            const int i = f0 + k;
            if (!depth[i] || (t->V.has_color && !color[i])) {
                gs2m_set_error("gs2m_tsdf_integrate_batch: frame %d has a NULL image", i);
                return 1;
            }
            const unsigned char* m = mask ? mask[i] : nullptr;
            if (fill_frame(t, hb[k].f, width, height, fx, fy, cx, cy, extrinsics_w2c + 16 * (size_t)i, depth_scale, depth_trunc,
                           min_depth, m != nullptr))
                return 1;
            hb[k].depth = depth[i];
            hb[k].color = color ? color[i] : nullptr;
            hb[k].mask = m;
        }
        GS2M_HIPCHK(hipMemcpyAsync(t->d_bframes.get(), hb, sizeof(TsdfBatchFrame) * nf, hipMemcpyHostToDevice, st));
        GS2M_HIPCHK(hipEventRecord(t->ring_done[slot], st));
        GS2M_HIPCHK(hipMemsetAsync(t->V.counters + 1, 0, sizeof(unsigned), st));  // touched_count = 0
        GS2M_HIPCHK(hipMemsetAsync(t->V.counters + 3, 0, sizeof(unsigned), st));  // work counter of the batch sweep
        {   // a batch counts as nf launches of each stage: the averages stay per frame
            StageTimer tm(t->events, t->timing != 0, st, 0, "gs2m:tsdf_touch_batch", nf);
            gs2m_launch_tsdf_touch_batch(st, t->V, hb[0].f, nf, t->d_bframes.get(), t->d_tiles.get());
        }
        {
            StageTimer tm(t->events, t->timing != 0, st, 1, "gs2m:tsdf_integrate_batch", nf);
            gs2m_launch_tsdf_integrate_batch(st, t->n_cu, t->V, t->d_bframes.get(), t->d_tiles.get());
        }
    }
    return 0;
}

extern "C" int gs2m_tsdf_set_stage_timing(gs2m_tsdf* t, int enable) {
    if (!t) {
        gs2m_set_error("null handle");
        return 1;
    }
    t->timing = enable != 0;
    return 0;
}

extern "C" int gs2m_tsdf_stage_times(gs2m_tsdf* t, gs2m_stream stream, double* total_ms, int64_t* launches) {
    if (!t || !total_ms || !launches) {
        gs2m_set_error("gs2m_tsdf_stage_times: NULL argument");
        return 1;
    }
    GS2M_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    t->events.drain(total_ms, launches, 2);   // a batch launch counts as its frames: averages stay per frame
    return 0;
}

extern "C" int gs2m_tsdf_status(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_blocks, int64_t* block_updates,
                                int* overflow) {
    if (!t) {
        gs2m_set_error("null handle");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    GS2M_HIPCHK(hipMemcpyAsync(t->h_counters.get(), t->V.counters, sizeof(unsigned) * 4, hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipMemcpyAsync(t->h_totals.get(), t->V.totals, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    GS2M_HIPCHK(hipGetLastError());
    unsigned nb = t->h_counters.get()[0];
    if (nb > t->V.max_blocks) nb = t->V.max_blocks;
    if (n_blocks) *n_blocks = nb;
    if (block_updates) *block_updates = (int64_t)t->h_totals.get()[0];
    if (overflow) *overflow = (int)t->h_counters.get()[2];
    return 0;
}

extern "C" int gs2m_tsdf_flags_device(gs2m_tsdf* t, uint32_t* flags_dev, gs2m_stream stream) {
    if (!t || !flags_dev) {
        gs2m_set_error("gs2m_tsdf_flags_device: NULL argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    GS2M_HIPCHK(hipMemcpyAsync(flags_dev, t->V.counters + 2, sizeof(unsigned), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int gs2m_tsdf_block_keys(gs2m_tsdf* t, int64_t n, int32_t* keys, gs2m_stream stream) {
    if (!t || (n > 0 && !keys) || n < 0 || n > (int64_t)t->V.max_blocks) {
        gs2m_set_error("gs2m_tsdf_block_keys: bad argument");
        return 1;
    }
    if (n == 0) return 0;
    GS2M_HIPCHK(hipSetDevice(t->device));
    gs2m_launch_tsdf_owned_keys((hipStream_t)stream, (unsigned)n, t->V, keys);   // halo copies -> sentinel key
    return 0;
}

// bytes of the exchange buffer of a window of dim[0] x dim[1] x dim[2] blocks and `world` ranks: the cells (one byte per block,
// rounded up to 16 so the header is aligned), then the header
static int64_t map_bytes(const int32_t* dim, int world, unsigned* n_cells_out) {
    if (!dim || dim[0] <= 0 || dim[1] <= 0 || dim[2] <= 0 || world <= 0) return -1;
    const int64_t cells = (int64_t)dim[0] * dim[1] * dim[2];
    if (cells > ((int64_t)1 << 30)) return -1;
    const unsigned nc = (unsigned)((cells + 15) / 16 * 16);
    if (n_cells_out) *n_cells_out = nc;
    return (int64_t)nc + GS2M_TSDF_MAP_HEADER_BYTES + 8 * (int64_t)world;
}

static unsigned window_hash(const int32_t* lo, const int32_t* dim) {
    unsigned h = 2166136261u;
    for (int k = 0; k < 3; ++k) {
        h = (h ^ (unsigned)lo[k]) * 16777619u;
        h = (h ^ (unsigned)dim[k]) * 16777619u;
    }
    return h;
}

extern "C" int64_t gs2m_tsdf_map_bytes(const int32_t* dim, int world) { return map_bytes(dim, world, nullptr); }

extern "C" int gs2m_tsdf_block_map(gs2m_tsdf* t, const int32_t* lo, const int32_t* dim, int rank, int world, int64_t frames_local,
                                   int64_t frames_base, int flags, uint8_t* cells, gs2m_stream stream) {
    unsigned nc = 0;
    const int64_t total = map_bytes(dim, world, &nc);
    if (!t || !lo || !cells || total < 0 || rank < 0 || rank >= world || frames_local < 0 || frames_base < 0 ||
        frames_local > 0x7fffffff || frames_base > 0x7fffffff) {
        gs2m_set_error("gs2m_tsdf_block_map: bad argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    GS2M_HIPCHK(hipMemsetAsync(cells, 0, (size_t)total, st));
    gs2m_launch_tsdf_block_map(st, t->V, lo, dim, cells, nc, (unsigned)flags, window_hash(lo, dim), rank, (unsigned)frames_local,
                               (unsigned)frames_base);
    GS2M_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gs2m_tsdf_map_keys(gs2m_tsdf* t, const int32_t* lo, const int32_t* dim, int world, uint8_t* cells, int32_t* keys,
                                  int64_t max_keys, uint8_t* header_host, gs2m_stream stream) {
    unsigned nc = 0;
    const int64_t total = map_bytes(dim, world, &nc);
    if (!t || !lo || !cells || total < 0 || max_keys < 0 || (max_keys > 0 && !keys) || !header_host) {
        gs2m_set_error("gs2m_tsdf_map_keys: bad argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    gs2m_launch_tsdf_map_keys(st, lo, dim, cells, nc, keys, (unsigned)(max_keys > 0x7fffffff ? 0x7fffffff : max_keys));
    GS2M_HIPCHK(hipGetLastError());
    GS2M_HIPCHK(hipMemcpyAsync(header_host, cells + nc, (size_t)(total - nc), hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int gs2m_tsdf_download(gs2m_tsdf* t, gs2m_stream stream, int64_t n, int32_t* keys, float* tsdf,
                                  float* weight, uint32_t* rgb_sum) {
    if (!t || n < 0) {
        gs2m_set_error("gs2m_tsdf_download: bad argument");
        return 1;
    }
    int64_t nb = 0;
    if (gs2m_tsdf_status(t, stream, &nb, nullptr, nullptr)) return 1;
    if (n > nb) n = nb;
    if (n == 0) return 0;
    const size_t nv = (size_t)n * GS2M_TSDF_VOX;
    if (keys) GS2M_HIPCHK(hipMemcpy(keys, t->V.block_keys, sizeof(int) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<float> tmp;
    // device layout (4x4x4 micro-blocks, tsdf_common.h)  ->  Open3D IndexOf x*256 + y*16 + z
    auto reorder_f = [&](const float* src, float* dst) {
        for (int64_t b = 0; b < n; ++b)
            for (int z = 0; z < 16; ++z)
                for (int x = 0; x < 16; ++x)
                    for (int y = 0; y < 16; ++y)
                        dst[(size_t)b * GS2M_TSDF_VOX + x * 256 + y * 16 + z] =
                            src[(size_t)b * GS2M_TSDF_VOX + GS2M_TSDF_VINDEX(x, y, z)];
    };
    if (tsdf) {
        tmp.resize(nv);
        GS2M_HIPCHK(hipMemcpy(tmp.data(), t->V.tsdf, sizeof(float) * nv, hipMemcpyDeviceToHost));
        reorder_f(tmp.data(), tsdf);
    }
    if (weight) {
        tmp.resize(nv);
        GS2M_HIPCHK(hipMemcpy(tmp.data(), t->V.weight, sizeof(float) * nv, hipMemcpyDeviceToHost));
        reorder_f(tmp.data(), weight);
    }
    if (rgb_sum) {
        if (!t->V.has_color) {
            memset(rgb_sum, 0, sizeof(uint32_t) * 3 * nv);
        } else {
            std::vector<unsigned> c(3 * nv);
            GS2M_HIPCHK(hipMemcpy(c.data(), t->V.rgb, sizeof(unsigned) * 3 * nv, hipMemcpyDeviceToHost));
            for (int64_t b = 0; b < n; ++b)
                for (int ch = 0; ch < 3; ++ch)
                    for (int z = 0; z < 16; ++z)
                        for (int x = 0; x < 16; ++x)
                            for (int y = 0; y < 16; ++y)
                                rgb_sum[((size_t)b * GS2M_TSDF_VOX + x * 256 + y * 16 + z) * 3 + ch] =
                                    c[((size_t)b * 3 + ch) * GS2M_TSDF_VOX + GS2M_TSDF_VINDEX(x, y, z)];
        }
    }
    return 0;
}

extern "C" int gs2m_tsdf_pack(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, float* buf_f32, int64_t* buf_i64,
                              gs2m_stream stream) {
    if (!t || n < 0 || form < 0 || form > 2 || (n > 0 && (!keys || !buf_f32 || (form == 2 && !buf_i64)))) {
        gs2m_set_error("gs2m_tsdf_pack: bad argument");
        return 1;
    }
    if (n == 0) return 0;
    GS2M_HIPCHK(hipSetDevice(t->device));
    gs2m_launch_tsdf_pack((hipStream_t)stream, (unsigned)n, t->V, keys, form, buf_f32, (long long*)buf_i64);
    return 0;
}

extern "C" int gs2m_tsdf_unpack(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, const float* buf_f32,
                                const int64_t* buf_i64, int halo, gs2m_stream stream) {
    if (!t || n < 0 || form < 0 || form > 2 || (n > 0 && (!keys || !buf_f32 || (form == 2 && !buf_i64)))) {
        gs2m_set_error("gs2m_tsdf_unpack: bad argument");
        return 1;
    }
    if (n == 0) return 0;
    GS2M_HIPCHK(hipSetDevice(t->device));
    gs2m_launch_tsdf_unpack((hipStream_t)stream, (unsigned)n, t->V, keys, form, buf_f32, (const long long*)buf_i64, halo);
    return 0;
}

extern "C" int gs2m_tsdf_replace(gs2m_tsdf* t, const int32_t* keys, int64_t n, int form, const float* buf_f32, const int64_t* buf_i64,
                                 gs2m_stream stream) {
    if (!t || n < 0 || (n > 0 && (!keys || !buf_f32))) {
        gs2m_set_error("gs2m_tsdf_replace: bad argument");
        return 1;
    }
    if (n > (int64_t)t->V.max_blocks) {
        gs2m_set_error("gs2m_tsdf_replace: block pool exhausted (%lld blocks to place, max_blocks = %u)", (long long)n, t->V.max_blocks);
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    // a reset that leaves the voxel state of the first n slots alone (they are overwritten by the unpack below, which hands out
    // exactly the slots [0, n) to n distinct in-range keys), then the unpack
    if (zero_state(t, (hipStream_t)stream, false, n)) return 1;
    if (n == 0) return 0;
    if (gs2m_tsdf_unpack(t, keys, n, form, buf_f32, buf_i64, 0, stream)) return 1;
    // keys that repeat / lie outside the key range / do not fit the hash table leave slots [counters[0], n) un-handed-out AND
    // un-cleared: cleared on the device (no host read; a no-op for n distinct in-range keys)
    gs2m_launch_tsdf_clear_gap((hipStream_t)stream, t->V, (unsigned)n);
    return 0;
}

extern "C" int gs2m_tsdf_pack_sum(gs2m_tsdf* t, const int32_t* keys, int64_t n, float* buf, gs2m_stream stream) {
    return gs2m_tsdf_pack(t, keys, n, 0, buf, nullptr, stream);
}

extern "C" int gs2m_tsdf_unpack_sum(gs2m_tsdf* t, const int32_t* keys, int64_t n, const float* buf, int halo,
                                    gs2m_stream stream) {
    return gs2m_tsdf_unpack(t, keys, n, 0, buf, nullptr, halo, stream);
}

extern "C" int gs2m_tsdf_extract_count(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_triangles) {
    if (!t || !n_triangles) {
        gs2m_set_error("gs2m_tsdf_extract_count: NULL argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    int64_t nb = 0;
    if (gs2m_tsdf_status(t, stream, &nb, nullptr, nullptr)) return 1;
    *n_triangles = 0;
    if (nb == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    gs2m_launch_mc_count(st, t->V, t->mc(), (unsigned)nb, t->d_blk_tris.get(), t->d_ntri.get());
    unsigned long long n = 0;
    GS2M_HIPCHK(hipMemcpyAsync(&n, t->d_ntri.get(), sizeof(n), hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    if (n >= (1ull << 32)) {
        gs2m_set_error("mesh too large: %llu triangles (32-bit per-block offsets)", n);
        return 1;
    }
    *n_triangles = (int64_t)n;
    return 0;
}

extern "C" int gs2m_tsdf_extract(gs2m_tsdf* t, gs2m_stream stream, int64_t max_triangles, double* vertices,
                                 double* colors, int64_t* n_triangles) {
    return gs2m_tsdf_extract_indexed(t, stream, max_triangles, vertices, colors, nullptr, n_triangles);
}

extern "C" int gs2m_tsdf_extract_indexed(gs2m_tsdf* t, gs2m_stream stream, int64_t max_triangles, double* vertices,
                                         double* colors, int32_t* edge_index, int64_t* n_triangles) {
    if (!t || !vertices || max_triangles < 0) {
        gs2m_set_error("gs2m_tsdf_extract: bad argument");
        return 1;
    }
    int64_t n = 0;
    if (gs2m_tsdf_extract_count(t, stream, &n)) return 1;  // (re)computes the per-block offsets
    if (n_triangles) *n_triangles = n;
    if (n == 0 || max_triangles == 0) return 0;
    int64_t nb = 0;
    if (gs2m_tsdf_status(t, stream, &nb, nullptr, nullptr)) return 1;
    gs2m_launch_mc_emit((hipStream_t)stream, t->V, t->mc(), (unsigned)nb, t->d_blk_tris.get(), (unsigned long long)max_triangles,
                        t->voxel_length, t->unit_length, vertices, colors, edge_index);
    return 0;
}

// ---- device-side mesh: extraction + welding, connected components ----------------------------------------------------------------
namespace {
unsigned pow2_at_least(unsigned long long n) {
    unsigned c = 1024u;
    while ((unsigned long long)c < n && c < 0x80000000u) c <<= 1;
    return c;
}
// gs2m_mesh_cluster / gs2m_mesh_vertex_normals have no handle: one arena per device, used under that device's lock (both
// calls synchronise before they return)
struct DeviceScratch {
    std::mutex lock;
    ScratchArena arena;
};
DeviceScratch& device_scratch(int device) {   // device in 0..63
    // Process lifetime: made on first use and never deleted.  As a static object the table would be destroyed at process
    // exit, and freeing device memory after the HIP runtime has shut down can crash or hang there.
    static DeviceScratch* const table = new DeviceScratch[64];
    return table[device];
}
}  // namespace

// forget the cached mesh (its arrays stay allocated: grow-only, freed with the handle)
static void drop_mesh(gs2m_tsdf* t) { t->mesh_nv = t->mesh_nt = 0; }

extern "C" int gs2m_tsdf_extract_mesh(gs2m_tsdf* t, gs2m_stream stream, int64_t* n_vertices, int64_t* n_triangles) {
    if (!t || !n_vertices || !n_triangles) {
        gs2m_set_error("gs2m_tsdf_extract_mesh: NULL argument");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    drop_mesh(t);
    *n_vertices = *n_triangles = 0;
    int64_t nt = 0;
    if (gs2m_tsdf_extract_count(t, stream, &nt)) return 1;
    if (nt == 0) return 0;
    if (nt > 0x2aaaaaaa) {
        gs2m_set_error("gs2m_tsdf_extract_mesh: %lld triangles exceed the 32-bit vertex numbering", (long long)nt);
        return 1;
    }
    const unsigned n = (unsigned)(3 * nt);
    const unsigned cap = pow2_at_least(2ull * n);
    const unsigned m = (n + 4095u) / 4096u;
    double *soup_v, *soup_c;
    int *soup_e, *small;
    unsigned long long* hkeys;
    unsigned *hfirst, *cell_of, *flag, *pos, *scratch;
    if (t->mesh_tri.reserve(n) ||
        t->mesh_scratch.carve(arena_sub(soup_v, 3 * (size_t)n), arena_sub(soup_c, 3 * (size_t)n), arena_sub(soup_e, 4 * (size_t)n),
                              arena_sub(hkeys, cap), arena_sub(hfirst, cap), arena_sub(cell_of, n), arena_sub(flag, n),
                              arena_sub(pos, n), arena_sub(scratch, (size_t)m + 2), arena_sub(small, 4))) {
        gs2m_set_error("gs2m_tsdf_extract_mesh: out of device memory for %lld triangles", (long long)nt);
        return 1;
    }
    int64_t nb = 0;
    if (gs2m_tsdf_status(t, stream, &nb, nullptr, nullptr)) return 1;
    gs2m_launch_mc_emit(st, t->V, t->mc(), (unsigned)nb, t->d_blk_tris.get(), (unsigned long long)nt, t->voxel_length, t->unit_length,
                        soup_v, soup_c, soup_e);
    const int init[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0};      // mins[3], bad
    GS2M_HIPCHK(hipMemcpyAsync(small, init, sizeof(init), hipMemcpyHostToDevice, st));
    GS2M_HIPCHK(hipMemsetAsync(hkeys, 0xff, sizeof(unsigned long long) * (size_t)cap, st));
    GS2M_HIPCHK(hipMemsetAsync(hfirst, 0xff, sizeof(unsigned) * (size_t)cap, st));
    // the compact arrays cannot be sized before the scan: first the flags, the scan and its total, then the (grow-only) arrays and the emit
    {
        int* mins = small;
        unsigned* bad = reinterpret_cast<unsigned*>(mins + 3);
        gs2m_launch_mesh_weld_count(st, n, soup_e, mins, hkeys, hfirst, cap, cell_of, flag, pos, scratch, bad);
        unsigned total = 0;
        int hb[4];
        GS2M_HIPCHK(hipMemcpyAsync(&total, scratch + m, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        GS2M_HIPCHK(hipMemcpyAsync(hb, small, sizeof(hb), hipMemcpyDeviceToHost, st));
        GS2M_HIPCHK(hipStreamSynchronize(st));
        if (hb[3]) {
            gs2m_set_error("gs2m_tsdf_extract_mesh: the surface spans more than 2^20 voxels along an axis (62-bit weld key)");
            drop_mesh(t);
            return 1;
        }
        if (t->mesh_v.reserve(3 * (size_t)total) || t->mesh_c.reserve(3 * (size_t)total) || t->mesh_e.reserve(4 * (size_t)total)) {
            gs2m_set_error("gs2m_tsdf_extract_mesh: out of device memory for %u vertices", total);
            return 1;
        }
        gs2m_launch_mesh_weld_emit(st, n, hfirst, cell_of, pos, soup_v, t->V.has_color ? soup_c : nullptr, soup_e, t->mesh_v.get(), t->mesh_c.get(),
                                   t->mesh_e.get(), t->mesh_tri.get());
        GS2M_HIPCHK(hipStreamSynchronize(st));
        GS2M_HIPCHK(hipGetLastError());
        t->mesh_nv = (int64_t)total;
        t->mesh_nt = nt;
    }
    *n_vertices = t->mesh_nv;
    *n_triangles = t->mesh_nt;
    return 0;
}

extern "C" int gs2m_tsdf_mesh_copy(gs2m_tsdf* t, gs2m_stream stream, double* vertices, double* colors, int32_t* edge_index, int32_t* triangles) {
    if (!t) {
        gs2m_set_error("null handle");
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    if (t->mesh_nv > 0) {
        if (vertices) GS2M_HIPCHK(hipMemcpyAsync(vertices, t->mesh_v.get(), sizeof(double) * 3 * (size_t)t->mesh_nv, hipMemcpyDefault, st));
        if (colors) GS2M_HIPCHK(hipMemcpyAsync(colors, t->mesh_c.get(), sizeof(double) * 3 * (size_t)t->mesh_nv, hipMemcpyDefault, st));
        if (edge_index) GS2M_HIPCHK(hipMemcpyAsync(edge_index, t->mesh_e.get(), sizeof(int) * 4 * (size_t)t->mesh_nv, hipMemcpyDefault, st));
    }
    if (t->mesh_nt > 0 && triangles) GS2M_HIPCHK(hipMemcpyAsync(triangles, t->mesh_tri.get(), sizeof(int) * 3 * (size_t)t->mesh_nt, hipMemcpyDefault, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int gs2m_mesh_cluster(int device, gs2m_stream stream, int64_t n_triangles, const int32_t* triangles, int32_t* labels,
                                 int64_t* cluster_n_triangles, int64_t* n_clusters) {
    if (n_triangles < 0 || n_triangles > 0x7fffffff || !n_clusters || (n_triangles > 0 && (!triangles || !labels || !cluster_n_triangles))) {
        gs2m_set_error("gs2m_mesh_cluster: bad argument");
        return 1;
    }
    *n_clusters = 0;
    if (n_triangles == 0) return 0;
    GS2M_HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)n_triangles;
    const unsigned cap = pow2_at_least(6ull * nt);
    const unsigned m = (nt + 4095u) / 4096u;
    if (device < 0 || device >= 64) {
        gs2m_set_error("gs2m_mesh_cluster: device %d not in 0..63", device);
        return 1;
    }
    DeviceScratch& ds = device_scratch(device);
    std::lock_guard<std::mutex> hold(ds.lock);
    unsigned long long* hkeys;
    unsigned *hval, *parent, *root, *flag, *pos, *scratch;
    if (ds.arena.carve(arena_sub(hkeys, cap), arena_sub(hval, cap), arena_sub(parent, nt), arena_sub(root, nt), arena_sub(flag, nt),
                       arena_sub(pos, nt), arena_sub(scratch, (size_t)m + 2))) {
        gs2m_set_error("gs2m_mesh_cluster: out of device memory for %u triangles", nt);
        return 1;
    }
    GS2M_HIPCHK(hipMemsetAsync(hkeys, 0xff, sizeof(unsigned long long) * (size_t)cap, st));
    GS2M_HIPCHK(hipMemsetAsync(hval, 0xff, sizeof(unsigned) * (size_t)cap, st));
    GS2M_HIPCHK(hipMemsetAsync(cluster_n_triangles, 0, sizeof(int64_t) * (size_t)nt, st));
    gs2m_launch_mesh_cluster(st, triangles, nt, hkeys, hval, cap, parent, root, flag, pos, scratch, labels,
                             reinterpret_cast<unsigned long long*>(cluster_n_triangles));
    unsigned total = 0;
    GS2M_HIPCHK(hipMemcpyAsync(&total, scratch + m, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    GS2M_HIPCHK(hipGetLastError());
    *n_clusters = (int64_t)total;
    return 0;
}

extern "C" int gs2m_mesh_vertex_normals(int device, gs2m_stream stream, int64_t n_vertices, const double* vertices, int64_t n_triangles,
                                        const int32_t* triangles, double* triangle_normals, double* vertex_normals) {
    if (n_vertices < 0 || n_vertices > 0x7fffffff || n_triangles < 0 || n_triangles > 0x2aaaaaaa || (n_vertices > 0 && !vertex_normals) ||
        (n_triangles > 0 && (!vertices || !triangles || !triangle_normals))) {
        gs2m_set_error("gs2m_mesh_vertex_normals: bad argument");
        return 1;
    }
    if (device < 0 || device >= 64) {
        gs2m_set_error("gs2m_mesh_vertex_normals: device %d not in 0..63", device);
        return 1;
    }
    if (n_vertices == 0 && n_triangles == 0) return 0;
    if (n_vertices == 0) {
        gs2m_set_error("gs2m_mesh_vertex_normals: %lld triangles and no vertices", (long long)n_triangles);
        return 1;
    }
    GS2M_HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) {
        GS2M_HIPCHK(hipMemsetAsync(vertex_normals, 0, sizeof(double) * 3 * (size_t)n_vertices, st));
        GS2M_HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    const unsigned nv = (unsigned)n_vertices, nt = (unsigned)n_triangles, ni = 3u * nt;
    const unsigned m = (nv + 4095u) / 4096u;
    DeviceScratch& ds = device_scratch(device);
    std::lock_guard<std::mutex> hold(ds.lock);
    unsigned *deg, *off, *fill, *list, *list2, *owner, *scratch;
    unsigned* small;      // {bad index, largest degree}
    if (ds.arena.carve(arena_sub(deg, nv), arena_sub(off, nv), arena_sub(fill, nv), arena_sub(list, ni), arena_sub(list2, ni),
                       arena_sub(owner, ni), arena_sub(scratch, (size_t)m + 2), arena_sub(small, 2))) {
        gs2m_set_error("gs2m_mesh_vertex_normals: out of device memory for %u triangles", nt);
        return 1;
    }
    GS2M_HIPCHK(hipMemsetAsync(deg, 0, sizeof(unsigned) * (size_t)nv, st));
    GS2M_HIPCHK(hipMemsetAsync(fill, 0, sizeof(unsigned) * (size_t)nv, st));
    GS2M_HIPCHK(hipMemsetAsync(small, 0, sizeof(unsigned) * 2, st));
    gs2m_launch_mesh_normals_bucket(st, vertices, nv, triangles, nt, triangle_normals, deg, off, fill, list, owner, scratch, small);
    unsigned h_small[2] = {0u, 0u};
    GS2M_HIPCHK(hipMemcpyAsync(h_small, small, sizeof(h_small), hipMemcpyDeviceToHost, st));
    GS2M_HIPCHK(hipStreamSynchronize(st));
    GS2M_HIPCHK(hipGetLastError());
    if (h_small[0]) {
        gs2m_set_error("gs2m_mesh_vertex_normals: a triangle names a vertex outside 0..%u", nv - 1);
        return 1;
    }
    for (unsigned width = 1u; width < h_small[1]; width *= 2u) {
        gs2m_launch_mesh_bucket_merge(st, ni, width, off, deg, owner, list, list2);
        unsigned* t = list;
        list = list2;
        list2 = t;
        if (width > 0x7fffffffu) break;
    }
    gs2m_launch_mesh_vertex_sum(st, nv, nt, off, deg, list, triangle_normals, vertex_normals);
    GS2M_HIPCHK(hipStreamSynchronize(st));
    GS2M_HIPCHK(hipGetLastError());
    return 0;
}
