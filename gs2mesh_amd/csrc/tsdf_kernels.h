// tsdf_kernels.h -- per-frame TSDF integration kernels (compiled with -ffp-contract=off).
//
// Reference path: volume.integrate(rgbd, intrinsic, inv(extrinsic)) (gs2mesh_utils/tsdf_utils.py:107)
// = Open3D 0.17 ScalableTSDFVolume::Integrate (restated in oracle/tsdf_oracle.cpp):
//   (i)  back-project every `stride`-th valid depth pixel to world space in fp64, mark every
//        16^3 block overlapping the +-sdf_trunc box of the point (first touch in this frame);
//   (ii) for each marked block sweep its 4096 voxels: project the voxel centre, fetch depth,
//        sdf = (d - z) * ||ray||, and where sdf > -trunc update the running means.
// Here: (i) = k_tsdf_touch (thread per strided pixel, wave-deduplicated block boxes, blocks
// found-or-inserted in a device hash table and stamped with the frame id) + k_tsdf_compact (stamped
// cells -> the frame's block list); (ii) = k_tsdf_integrate, one 256-thread workgroup per touched
// block (grid-stride over the device-side list: no host sync between the phases), sweeping the
// block's 4x4x4 micro-blocks with the same fp32 camera-space z chain as upstream (replayed from the
// column start, so every rounding matches).
// The RGBD conversion (depth/scale, >= trunc -> 0; RGBDImage.create_from_color_and_depth,
// tsdf_utils.py:88-93) and TSDF.run's mask / min-depth preprocessing (tsdf_utils.py:68-83) are
// fused into the depth fetch.
#pragma once
#include "tsdf_common.h"

// ---- the Open3D voxel update, each step stated once ---------------------------------------------------------------------------
// UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier + the RGBD conversion in front of it.  k_tsdf_integrate,
// k_tsdf_integrate_batch and the touch kernels are put together from these steps and from nothing else: that the batch call
// gives the bits of the frame-by-frame calls rests on both running THIS arithmetic, in this order (no contraction: the
// translation unit is compiled with -ffp-contract=off).

// camera-space centre of the voxel whose world-space centre is (p0, p1, p2)
GS2M_DEVICE void tsdf_cam_point(const TsdfFrame& f, float p0, float p1, float p2, float& pc0, float& pc1, float& pc2) {
    pc0 = f.E[0] * p0 + f.E[1] * p1 + f.E[2] * p2 + f.E[3] * 1.f;
    pc1 = f.E[4] * p0 + f.E[5] * p1 + f.E[6] * p2 + f.E[7] * 1.f;
    pc2 = f.E[8] * p0 + f.E[9] * p1 + f.E[10] * p2 + f.E[11] * 1.f;
}
// one voxel further along z: upstream advances the point by repeated fp32 addition, so the rounding accumulates along z
GS2M_DEVICE void tsdf_z_step(const TsdfFrame& f, float& pc0, float& pc1, float& pc2) {
    pc0 += f.Es02;
    pc1 += f.Es12;
    pc2 += f.Es22;
}
// pixel (u, v) the point projects to; returns v * W + u, or -1 (u, v untouched) behind the camera or off the image.  A NaN z
// is not rejected by `pc2 <= 0`: it goes on and fails the bounds.
GS2M_DEVICE int tsdf_project(const TsdfFrame& f, float pc0, float pc1, float pc2, int& u, int& v) {
    if (pc2 <= 0) return -1;
    const float u_f = pc0 * f.fx_f / pc2 + f.cx_f + 0.5f;
    const float v_f = pc1 * f.fy_f / pc2 + f.cy_f + 0.5f;
    if (!(u_f >= 0.0001f && u_f < f.safe_w && v_f >= 0.0001f && v_f < f.safe_h)) return -1;
    u = (int)u_f;
    v = (int)v_f;
    return v * f.W + u;
}
// Image::CreateDepthToCameraDistanceMultiplierFloatImage at pixel (u, v), evaluated on the fly
GS2M_DEVICE float tsdf_distance_multiplier(const TsdfFrame& f, int u, int v) {
    const float xx = (u - f.cx_f) * f.fx_inv_f;
    const float yy = (v - f.cy_f) * f.fy_inv_f;
    return sqrtf(xx * xx + yy * yy + 1.0f);
}
// Depth as the integrator sees it (tsdf_utils.py:68-93 + Image::ConvertDepthToFloatImage), in two halves: the load with
// TSDF.run's mask, then the conversion.  The batch sweep runs them a frame apart, everything else back to back.
GS2M_DEVICE float tsdf_mask_depth(float d, unsigned mask_byte) {
    return mask_byte == 0u ? d * 0.0f : d;                   // depth = depth * mask  (a NaN or infinite depth stays NaN)
}
GS2M_DEVICE float tsdf_read_depth(const TsdfFrame& f, const float* __restrict__ depth, const unsigned char* __restrict__ mask, size_t pix) {
    float d = depth[pix];
    if (f.use_mask) d = tsdf_mask_depth(d, mask[pix]);
    return d;
}
GS2M_DEVICE float tsdf_convert_depth(const TsdfFrame& f, float d) {
    if (f.use_min && d < f.min_depth_f) d = 0.0f;            // depth[depth < min] = 0
    if (f.depth_scale_f != 1.0f) d /= f.depth_scale_f;       // *p /= (float)depth_scale (x / 1 == x: skipped, uniform)
    if (d >= f.depth_trunc_up_f) d = 0.0f;                   // if (*p >= depth_trunc) *p = 0  (float vs double threshold, exactly)
    return d;
}
// does depth d, seen from a voxel at camera-space z `zc` under distance multiplier `mult`, update the voxel?  tnew = its sample
GS2M_DEVICE bool tsdf_decide(const TsdfFrame& f, float d, float zc, float mult, float& tnew) {
    const float sdf = (d - zc) * mult;
    tnew = fminf(1.0f, sdf * f.sdf_trunc_inv_f);
    return d > 0.0f && sdf > -f.sdf_trunc_f;
}
// r | g << 8 | b << 16 of pixel `pix` in ONE gather (the 4th byte belongs to the next pixel; the last pixel of the image is
// read bytewise so that nothing past the buffer is touched)
GS2M_DEVICE unsigned tsdf_gather_rgb(const unsigned char* __restrict__ color, int pix, int last_pix) {
    const unsigned char* c = color + 3 * (size_t)pix;
    return pix < last_pix ? gs2m_load_u32_unaligned(c) : ((unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16));
}
// the running mean takes the sample, the colour sums (volumes with colour only) take the pixel
GS2M_DEVICE void tsdf_update_mean(float& t, float& w, float tnew) {
    t = (t * w + tnew) / (w + 1.0f);
    w = w + 1.0f;
}
GS2M_DEVICE void tsdf_update_rgb(unsigned& c0, unsigned& c1, unsigned& c2, unsigned rgbp) {
    c0 += rgbp & 0xffu;
    c1 += (rgbp >> 8) & 0xffu;
    c2 += (rgbp >> 16) & 0xffu;
}
// The voxel-centre coordinates of the block with hash key `key` (no dependent block_keys load): threads 0..15 write the 16 x
// coordinates to s_p0, threads 16..31 the 16 y coordinates to s_p1 (the caller's barriers go around this), all get the z
// coordinate of the block's first plane.  fp64 add + cast as upstream: float(half + vl * i + origin), with
// OpenVolumeUnit's origin = index.cast<double>() * volume_unit_length.
GS2M_DEVICE float tsdf_block_centres(const TsdfFrame& f, unsigned long long key, int tid, float* s_p0, float* s_p1) {
    int bx, by, bz;
    tsdf_unpack_key(key, bx, by, bz);
    const double ox = (double)bx * f.unit_length, oy = (double)by * f.unit_length, oz = (double)bz * f.unit_length;
    if (tid < 16) s_p0[tid] = (float)(f.half_voxel_length_f + f.voxel_length_f * tid + ox);
    else if (tid < 32) s_p1[tid - 16] = (float)(f.half_voxel_length_f + f.voxel_length_f * (tid - 16) + oy);
    return (float)(f.half_voxel_length_f + oz);
}

// find-or-insert `key`; returns the hash index or 0xffffffff on failure (table full)
GS2M_DEVICE unsigned tsdf_find_or_insert(const TsdfVolume& V, unsigned long long key, int bx, int by, int bz) {
    const unsigned mask = V.hash_cap - 1u;
    unsigned h = tsdf_hash(key) & mask;
    for (unsigned probe = 0; probe < V.hash_cap; ++probe, h = (h + 1u) & mask) {
        unsigned long long k = V.hash_keys[h];
        if (k == key) return h;
        if (k == GS2M_TSDF_EMPTY) {
            const unsigned long long prev = atomicCAS(&V.hash_keys[h], GS2M_TSDF_EMPTY, key);
            if (prev == GS2M_TSDF_EMPTY) {
                // we inserted: take a pool slot (the pool is zero-initialised = a fresh Open3D unit)
                const unsigned slot = atomicAdd(&V.counters[0], 1u);
                if (slot < V.max_blocks) {
                    V.block_keys[3 * (size_t)slot] = bx;
                    V.block_keys[3 * (size_t)slot + 1] = by;
                    V.block_keys[3 * (size_t)slot + 2] = bz;
                    V.hash_vals[h] = (int)slot;
                } else {
                    atomicOr(&V.counters[2], 1u);  // pool exhausted
                }
                return h;
            }
            if (prev == key) return h;
            // somebody else took the cell for another key: keep probing
        }
    }
    atomicOr(&V.counters[2], 2u);  // hash table full
    return 0xffffffffu;
}

// read-only lookup: slot or -1
GS2M_DEVICE int tsdf_lookup(const TsdfVolume& V, unsigned long long key) {
    const unsigned mask = V.hash_cap - 1u;
    unsigned h = tsdf_hash(key) & mask;
    for (unsigned probe = 0; probe < V.hash_cap; ++probe, h = (h + 1u) & mask) {
        const unsigned long long k = V.hash_keys[h];
        if (k == key) return V.hash_vals[h];
        if (k == GS2M_TSDF_EMPTY) return -1;
    }
    return -1;
}

// k_tsdf_touch: one thread per strided pixel back-projects its point (fp64, as upstream) and gets the
// block box [lo, hi] of its +-trunc cube (up to 27 blocks with the reference defaults).  Neighbouring
// pixels share almost all of those blocks -- a frame marks ~2 k distinct blocks out of ~3 M
// (point, block) pairs -- and every hash probe is a random L2 request, so the pairs are deduplicated
// per wave first: the 64 boxes go to LDS, the wave takes the union box, lane l tests candidate
// block base + l of the union against the 64 boxes (LDS broadcast reads) and only then probes the
// hash table.  ~50x fewer probes / stamp atomics than one probe per (point, block).
struct TouchStage {
    int lo[3][64];
    int hi[3][64];
};

GS2M_DEVICE int wave_min_i(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int o = gs2m_shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
GS2M_DEVICE int wave_max_i(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int o = gs2m_shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// BATCH_BIT < 0: per-frame mode, the touched hash cell is stamped with the frame id; >= 0: batch mode, bit BATCH_BIT of
// the cell's frame mask is set.
GS2M_DEVICE void tsdf_touch_body(const TsdfVolume& V, const TsdfFrame& f, const float* __restrict__ depth,
                                 const unsigned char* __restrict__ mask, TouchStage* stage_all, int batch_bit) {
    const int lane = (int)(threadIdx.x & 63u);
    TouchStage* stg = &stage_all[threadIdx.x >> 6];
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
    bool valid = false;
    if (idx < f.nx * f.ny) {
        const int i = (idx / f.nx) * f.stride;  // row
        const int j = (idx % f.nx) * f.stride;  // column
        const float p = tsdf_convert_depth(f, tsdf_read_depth(f, depth, mask, (size_t)i * f.W + j));
        if (p > 0.0f) {
            valid = true;
            // PointCloudFactory.cpp CreatePointCloudFromFloatDepthImage (fp64)
            const double z = (double)p;
            const double x = (j - f.cx) * z / f.fx;
            const double y = (i - f.cy) * z / f.fy;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double pw = f.pose[4 * r + 0] * x + f.pose[4 * r + 1] * y + f.pose[4 * r + 2] * z + f.pose[4 * r + 3] * 1.0;
                // ScalableTSDFVolume::LocateVolumeUnit: floor(p / volume_unit_length)
                lo[r] = (int)floor((pw - f.sdf_trunc) / f.unit_length);
                hi[r] = (int)floor((pw + f.sdf_trunc) / f.unit_length);
            }
        }
    }
    if (gs2m_ballot(valid ? 1 : 0) == 0ull) return;  // wave-uniform
    int wlo[3], whi[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        wlo[r] = wave_min_i(lo[r]);
        whi[r] = wave_max_i(hi[r]);
    }
    // Neighbouring pixels mostly have the SAME block box (a +-trunc cube is ~1.3 blocks wide, 64 strided pixels span ~5): only the
    // boxes that differ from the previous lane's are staged (round 4: typically 5-15 of 64), so the containment loop below runs
    // over the distinct boxes instead of all 64 lanes.  The union of the kept boxes is the union of all boxes: same block set.
    bool same = lane > 0 && valid;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int plo = gs2m_shfl_up(lo[r], 1), phi = gs2m_shfl_up(hi[r], 1);
        same = same && plo == lo[r] && phi == hi[r];
    }
    const bool pvalid = gs2m_shfl_up(valid ? 1 : 0, 1) != 0;
    const bool keep = valid && !(same && pvalid);
    const unsigned long long kept = gs2m_ballot(keep ? 1 : 0);
    const int n_keep = gs2m_popc64(kept);
    if (keep) {
        const int slot = gs2m_popc64(kept & ((1ull << lane) - 1ull));
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            stg->lo[r][slot] = lo[r];
            stg->hi[r][slot] = hi[r];
        }
    }
    gs2m_wave_sync();
    const long long total_ll = ((long long)whi[0] - wlo[0] + 1) * ((long long)whi[1] - wlo[1] + 1) *
                               ((long long)whi[2] - wlo[2] + 1);
    if (total_ll > (1ll << 24)) {  // a wave spanning > 16 M blocks: not a depth map of this volume
        if (lane == 0) atomicOr(&V.counters[2], 4u);
        return;
    }
    const int ny = whi[1] - wlo[1] + 1, nz = whi[2] - wlo[2] + 1;
    const int nyz = ny * nz;
    const int total = (int)total_ll;
    for (int base = 0; base < total; base += 64) {
        const int c = base + lane;
        if (c >= total) continue;
        const int cx = c / nyz, rem = c - cx * nyz;
        const int cy = rem / nz;
        const int bx = wlo[0] + cx, by = wlo[1] + cy, bz = wlo[2] + (rem - cy * nz);
        // containment in ANY staged box: branch-free so the broadcast LDS reads pipeline
        int in_any = 0;
#pragma unroll 4
        for (int k = 0; k < n_keep; ++k)
            in_any |= (int)(bx >= stg->lo[0][k]) & (int)(bx <= stg->hi[0][k]) & (int)(by >= stg->lo[1][k]) &
                      (int)(by <= stg->hi[1][k]) & (int)(bz >= stg->lo[2][k]) & (int)(bz <= stg->hi[2][k]);
        const bool inside = in_any != 0;
        if (!inside) continue;
        if (!tsdf_key_in_range(bx, by, bz)) {
            atomicOr(&V.counters[2], 4u);
            continue;
        }
        const unsigned h = tsdf_find_or_insert(V, tsdf_pack_key(bx, by, bz), bx, by, bz);
        if (h == 0xffffffffu) continue;
        // mark "touched in this frame" (touched_volume_units_ of upstream).  No list append here: ~2 k
        // returning atomics on ONE counter serialise at ~12 ns each (guide: fanin); k_tsdf_compact builds
        // the list with one atomic per 1024 hash cells instead.
        if (batch_bit < 0) {
            if (V.stamp[h] != f.frame_id) V.stamp[h] = f.frame_id;
        } else {
            const unsigned long long bit = 1ull << batch_bit;
            if (!(V.fmask[h] & bit)) atomicOr(&V.fmask[h], bit);
        }
    }
}

GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_touch(TsdfVolume V, TsdfFrame f, const float* __restrict__ depth, const unsigned char* __restrict__ mask) {
    __shared__ TouchStage stage_all[4];
    tsdf_touch_body(V, f, depth, mask, stage_all, -1);
}

// batch mode: k_tsdf_touch_batch, below the sweep's max-depth map it also builds


// Compacts the hash cells stamped in this frame into V.touched (order = hash order).
// frame_id == 0: batch mode -- cells whose frame mask is non-zero.
GS2M_KERNEL void __launch_bounds__(1024)
k_tsdf_compact(TsdfVolume V, unsigned frame_id) {
    __shared__ unsigned wave_cnt[16];
    __shared__ unsigned wg_base;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned h = blockIdx.x * 1024u + (unsigned)tid;
    const bool t = h < V.hash_cap && (frame_id ? V.stamp[h] == frame_id : V.fmask[h] != 0ull);
    const unsigned long long m = gs2m_ballot(t ? 1 : 0);
    if (lane == 0) wave_cnt[wave] = (unsigned)gs2m_popc64(m);
    __syncthreads();
    if (tid == 0) {
        unsigned s = 0;
        for (int k = 0; k < 16; ++k) {
            const unsigned c = wave_cnt[k];
            wave_cnt[k] = s;
            s += c;
        }
        wg_base = s ? atomicAdd(&V.counters[1], s) : 0u;
    }
    __syncthreads();
    if (t) {
        const unsigned rank = (unsigned)gs2m_popc64(m & ((1ull << lane) - 1ull));
        V.touched[wg_base + wave_cnt[wave] + rank] = h;
    }
}

// k_tsdf_integrate: one 256-thread workgroup per touched block (grid-stride over the device-side
// list).  Wave w, lane l sweep the block's 64 micro-blocks of 4x4x4 voxels (tsdf_common.h), four
// micro-blocks in flight per wave: all projections first (pure ALU), then all depth gathers, then all
// state loads + colour gathers, then the stores = ~4 dependent memory round trips per 4 micro-blocks.
// The camera-space point of a voxel is advanced along z by repeated fp32 addition exactly as upstream
// does (rounding accumulates along z), so a lane replays the z steps below its voxel.
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_integrate(TsdfVolume V, TsdfFrame f, const float* __restrict__ depth, const unsigned char* __restrict__ color,
                 const unsigned char* __restrict__ mask) {
    __shared__ float s_p0[16], s_p1[16];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lz = lane >> 4, lx = (lane >> 2) & 3, ly = lane & 3;
    const unsigned n_touched = V.counters[1];
    const int last_pix = f.W * f.H - 1;
    for (unsigned it = blockIdx.x; it < n_touched; it += gridDim.x) {
        const unsigned h = V.touched[it];
        const unsigned long long key = V.hash_keys[h];
        const int slot = V.hash_vals[h];
        if (slot < 0) continue;  // pool overflow (flagged); uniform across the workgroup
        __syncthreads();  // previous block's readers are done
        const float p2 = tsdf_block_centres(f, key, tid, s_p0, s_p1);
        __syncthreads();
        float* bt = V.tsdf + (size_t)slot * GS2M_TSDF_VOX;
        float* bw = V.weight + (size_t)slot * GS2M_TSDF_VOX;
        unsigned* bc = V.rgb + (size_t)slot * 3 * GS2M_TSDF_VOX;
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            int pix[4], vi[4];
            float zc[4], mult[4], d[4], tnew[4];
            // (a) projections.  g is the micro-block z index for all four k: mb = g*16 + wave*4 + k
            const int z0 = g * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int mb = g * 16 + wave * 4 + k;  // micro-block (mz = g, mx = wave, my = k)
                const int x = wave * 4 + lx, y = k * 4 + ly;
                vi[k] = mb * 64 + lane;
                float pc0, pc1, pc2;
                tsdf_cam_point(f, s_p0[x], s_p1[y], p2, pc0, pc1, pc2);
                // replay the z steps below this voxel: z0 wave-uniform steps, then lz (0..3) of its own
                for (int s = 0; s < z0; ++s) tsdf_z_step(f, pc0, pc1, pc2);
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (s < lz) tsdf_z_step(f, pc0, pc1, pc2);
                }
                int u = 0, v = 0;
                pix[k] = tsdf_project(f, pc0, pc1, pc2, u, v);
                zc[k] = pc2;
                mult[k] = pix[k] >= 0 ? tsdf_distance_multiplier(f, u, v) : 0.0f;
            }
            // (b) depth gathers, back to back
#pragma unroll
            for (int k = 0; k < 4; ++k)
                d[k] = pix[k] >= 0 ? tsdf_convert_depth(f, tsdf_read_depth(f, depth, mask, (size_t)pix[k])) : 0.0f;
            // (c) decide
            bool upd[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool hit = tsdf_decide(f, d[k], zc[k], mult[k], tnew[k]);
                upd[k] = pix[k] >= 0 && hit;
            }
            // (d) state loads + colour gathers
            float w[4], t[4];
            unsigned c0[4], c1[4], c2[4], rgbp[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (upd[k]) {
                    w[k] = bw[vi[k]];
                    t[k] = bt[vi[k]];
                    if (V.has_color) {
                        c0[k] = bc[vi[k]];
                        c1[k] = bc[GS2M_TSDF_VOX + vi[k]];
                        c2[k] = bc[2 * GS2M_TSDF_VOX + vi[k]];
                        rgbp[k] = tsdf_gather_rgb(color, pix[k], last_pix);
                    }
                }
            }
            // (e) update + stores
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (upd[k]) {
                    tsdf_update_mean(t[k], w[k], tnew[k]);
                    bt[vi[k]] = t[k];
                    if (V.has_color) {
                        tsdf_update_rgb(c0[k], c1[k], c2[k], rgbp[k]);
                        bc[vi[k]] = c0[k];
                        bc[GS2M_TSDF_VOX + vi[k]] = c1[k];
                        bc[2 * GS2M_TSDF_VOX + vi[k]] = c2[k];
                    }
                    bw[vi[k]] = w[k];
                }
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) V.totals[0] += n_touched;
}

// k_tsdf_integrate_batch: the frames of a batch in ONE sweep over the touched blocks, voxel-stationary (SURVEY.md 7,
// step 6 iii).  A 256-thread workgroup owns an x-quarter xq of a block, wave w its micro-column (xq, yq = w): the 4 micro-blocks
// stacked along z.  Lane (lz, lx, ly) -- laid out as in k_tsdf_integrate -- keeps the state of its position in each of them, the 4
// voxels (4 xq + lx, 4 w + ly, 4 j + lz), j = 0 .. 3, in registers (20 words).  So gather instruction j of a wave covers exactly
// micro-block (j, xq, w), the compact pixel patch the storage order was chosen for (tsdf_common.h), and a state load or store
// of it is 256 contiguous bytes per array.  The thread walks the frames that touched the block IN FRAME ORDER (bit f of the
// block's frame mask; Open3D integrates a block for a frame only if that frame's points touch it) and applies exactly the
// per-frame update (same fp32 sequence, same incremental z chain: per frame the point of voxel (x, y, 0) is advanced by lz
// steps to the thread's first voxel, then by 4 steps from each voxel to the next -- 15 steps = 45 additions per thread and frame,
// as many as the longest replay of the per-frame kernel's lane and in the same order) -- results are bit-identical to calling
// k_tsdf_integrate frame by frame.  Compared with the per-frame kernel: the voxel state is read and written once per batch
// instead of once per frame (40 B x updated voxels x frames -> 20 B x voxels of touched blocks), the distance multiplier (a
// correctly rounded sqrt) only where a depth sample exists, frame uniforms by scalar loads.
// Four work items per block (round 3; the round-2 form, one 1024-thread workgroup per block at 94 VGPRs = 4 waves per SIMD, was
// removed in round 4): finer items for the dynamic hand-out, and the block's frame mask is cleared by k_tsdf_clear_fmask
// afterwards (the four quarters of a block run on different workgroups).
// The lane mapping (profiles/tsdf_sweep_layout.txt; C2 / C4, us per frame in sweeps of 20, builds interleaved in one process):
// until this form a workgroup owned a z-quarter and thread (x, y) a run of 4 voxels along z, so one gather covered a 4 x 16
// slice of a z-plane, 2.2x the cache lines of a micro-block (tools/tsdf_gather_lines.py): 28.4 / 67.2.  The same runs with
// the wave over 8 x 8 of a z-plane: 25.8 / 63.0.  This mapping: 24.6 / 61.0 at 92 VGPRs.  A pending probe keeps neither the
// pixel index (v * W + u is formed again from the packed (u, v) for the colour gather; NO_PIXEL marks a voxel that sees no
// pixel) nor the 4 camera-space depths (one start value, the chain's additions are repeated on it): either one alone leaves
// the time where it was (84 VGPRs, still 5 waves per SIMD: 24.6 / 61.8, 24.4 / 61.2), both give 74 VGPRs = 6 waves per SIMD
// without a register cap or a spill: 23.5 / 58.5.  In the benchmark's own stage timing the sweep costs 21.7 us per frame on C2 and
// 59.7 on C4 (27.8 and 75.5 before); the bytes to HBM are what they were, 59 % of the vector-L1 line accesses are gone.
// Measured and not kept: the two squares of the distance multiplier from LDS tables over the image's columns and rows (16 KiB
// per workgroup) 24.2 -> 23.7 on C2 with rounds won and lost alike, 58.9 -> 58.0 on C4, and on the 92-VGPR form 24.7 -> 24.9 /
// 60.8 -> 61.7: no gain that stands out of the run-to-run spread (0.3 - 0.5 us).  Round 3, forcing 6 / 7 waves per SIMD with a
// register cap (80 / 72 VGPRs, spills) gained nothing.  Round 4 (profiles/r4_experiments.txt): the frames of a block probed four
// at a time by the four waves of the workgroup ("frame lanes": LDS exchange + barrier per round, one voxel of state per thread)
// 30 -> 80 us per frame -- the dependent round trips only move from the frame loop to a loop over x-quarters; the colour gathered
// together with the depth (one round trip per frame instead of two dependent ones, but for every probed voxel) 30.5 -> 35.2.
// The kernel itself follows the cull test it runs per work item:
//
// Frame passes proven dead by a max-depth map.  The touch rule marks every block in the +-sdf_trunc box of a depth sample, so
// many marked blocks lie beside the silhouette (every depth they see is 0) or wholly behind the band (every sdf <= -trunc):
// tools/tsdf_dead_pass_census.py counts 39 % (C2) and 30 % (C4) of the benchmark's wave passes as provably dead.  A culled pass
// issues no gather at all.
//
// The map, once per batch (k_tsdf_touch_batch): per frame and tile of 8 x 8 pixels the largest depth the integrator would accept (d > 0
// after mask, min_depth, depth_scale and depth_trunc; NaN, negative, zero, masked and truncated samples are no samples), 0 for a
// tile without one.  A wave takes 256 columns x 8 rows = 32 tiles, a workgroup four such spans side by side.  The kernel streams
// every depth image of the batch once, so it reads 16 bytes per lane where the rows allow it (the width a multiple of 4, the
// image 16-byte and the mask 4-byte aligned: 4 columns per lane, two lanes per tile, 8 loads in flight) and one float per lane
// in four 64-column steps otherwise.
GS2M_DEVICE float tsdf_tile_sample(const TsdfFrame& f, float m, float raw) {
    const float d = tsdf_convert_depth(f, raw);
    return d > 0.0f && d > m ? d : m;   // tsdf_decide's own test of a sample: a NaN never gets in
}
// tile row `ty` of frame `bf`, columns from 1024 * `bx`: `out` = that row of the frame's map
GS2M_DEVICE void tsdf_depth_tiles_body(const TsdfBatchFrame& bf, float* __restrict__ out, int bx, int ty) {
    const TsdfFrame& f = bf.f;
    const float* __restrict__ depth = bf.depth;
    const unsigned char* __restrict__ mask = bf.mask;
    const int lane = (int)(threadIdx.x & 63u);
    const int xw = (bx * 4 + (int)(threadIdx.x >> 6)) * 256;   // the wave's first column
    if (xw >= f.W) return;                                      // wave-uniform
    const int y0 = ty * GS2M_TSDF_TILE;
    const bool wide = (f.W & 3) == 0 && ((size_t)depth & 15u) == 0u && (!f.use_mask || ((size_t)mask & 3u) == 0u);
    if (wide) {
        const int x = xw + 4 * lane;
        float m = 0.0f;
        if (x < f.W) {
            float4 raw[GS2M_TSDF_TILE];
            unsigned mk[GS2M_TSDF_TILE];
#pragma unroll
            for (int r = 0; r < GS2M_TSDF_TILE; ++r) {
                const int y = y0 + r < f.H ? y0 + r : f.H - 1;   // below the image: the last row again
                const size_t pix = (size_t)y * f.W + x;
                raw[r] = *reinterpret_cast<const float4*>(depth + pix);
                mk[r] = f.use_mask ? *reinterpret_cast<const unsigned*>(mask + pix) : 0xffffffffu;
            }
#pragma unroll
            for (int r = 0; r < GS2M_TSDF_TILE; ++r) {
                m = tsdf_tile_sample(f, m, tsdf_mask_depth(raw[r].x, mk[r] & 0xffu));
                m = tsdf_tile_sample(f, m, tsdf_mask_depth(raw[r].y, (mk[r] >> 8) & 0xffu));
                m = tsdf_tile_sample(f, m, tsdf_mask_depth(raw[r].z, (mk[r] >> 16) & 0xffu));
                m = tsdf_tile_sample(f, m, tsdf_mask_depth(raw[r].w, mk[r] >> 24));
            }
        }
        const float o = gs2m_shfl_xor(m, 1);   // every lane takes part, also those right of the image (m = 0)
        if (o > m) m = o;
        if ((lane & 1) == 0 && x < f.W) out[x / GS2M_TSDF_TILE] = m;
        return;
    }
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int x = xw + 64 * i + lane;
        float m = 0.0f;
        if (x < f.W) {
#pragma unroll
            for (int r = 0; r < GS2M_TSDF_TILE; ++r) {
                const int y = y0 + r < f.H ? y0 + r : f.H - 1;
                m = tsdf_tile_sample(f, m, tsdf_read_depth(f, depth, mask, (size_t)y * f.W + x));
            }
        }
#pragma unroll
        for (int s = 1; s < GS2M_TSDF_TILE; s <<= 1) {
            const float o = gs2m_shfl_xor(m, s);
            if (o > m) m = o;
        }
        if ((lane & (GS2M_TSDF_TILE - 1)) == 0 && x < f.W) out[x / GS2M_TSDF_TILE] = m;
    }
}

// The touch pass of a batch and its map in ONE launch: blockIdx.y = frame of the batch; the first `n_touch` workgroups of a
// frame run the touch pass (bound by the latency of its hash probes), the others stream the frame's depth image into the map
// (bound by bandwidth), `map_wg_x` workgroups per tile row.  Both only read the images, neither reads what the other writes.
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_touch_batch(TsdfVolume V, const TsdfBatchFrame* __restrict__ frames, unsigned n_touch, float* __restrict__ tiles, int tiles_x,
                   int tiles_y, unsigned map_wg_x) {
    __shared__ TouchStage stage_all[4];
    const TsdfBatchFrame& bf = frames[blockIdx.y];
    if (blockIdx.x < n_touch) {
        tsdf_touch_body(V, bf.f, bf.depth, bf.mask, stage_all, (int)blockIdx.y);
    } else {
        const unsigned m = blockIdx.x - n_touch, ty = m / map_wg_x;
        tsdf_depth_tiles_body(bf, tiles + ((size_t)blockIdx.y * tiles_y + ty) * tiles_x, (int)(m - ty * map_wg_x), (int)ty);
    }
}

// Can frame `e4` (its E, three float4) update a voxel of the micro-column x in [xa, xb], y in [ya, yb] (voxel centres, world),
// z = z0 .. z0 + 15 voxels?  false only with a proof that it cannot:
//   * all 8 corner centres lie in front of the camera, so the column projects into the hull of its projected corners;
//   * F = the bounding box of the 8 projections, widened by mu >= 1 pixel (the + 0.5f truncation of tsdf_project, and the
//     distance of any voxel's computed point from the hull of these corners, below) and clipped to the image, is empty -- no
//     voxel sees a pixel -- or holds no depth sample (Dmax = the largest tile value over F is 0), or
//   * Dmax - zlow <= -sdf_trunc, zlow = the least corner z lowered by a voxel length and eps.
// tsdf_decide updates iff d > 0 && (d - zc) * mult > -trunc; every voxel of the column has d <= Dmax and zc >= zlow, fp32
// subtraction and multiplication are monotone and mult = sqrtf(1 + ...) >= 1 does not raise a difference that is <= 0: a
// culled pass would have updated nothing, and the volume keeps the bits of the uncut sweep.
// eps bounds how far a point the sweep computes (tsdf_cam_point, then up to 15 tsdf_z_steps: < 24 roundings of at most
// 2^-24 S each, S = the sum of the magnitudes of the terms) and a corner computed here (< 10 such) lie from the exact affine
// image of the voxel centre: 2^-18 S for both together.  A pose with a NaN or an infinity fails a comparison and is live.
GS2M_DEVICE bool tsdf_pass_live(const TsdfFrame& f0, const float4* __restrict__ e4, const float* __restrict__ tiles, int tiles_x,
                                float xa, float xb, float ya, float yb, float z0) {
    const float4 r0 = e4[0], r1 = e4[1], r2 = e4[2];
    const float vl = f0.voxel_length_f, zspan = 15.0f * vl;
    const float ax = fmaxf(fabsf(xa), fabsf(xb)), ay = fmaxf(fabsf(ya), fabsf(yb)), az = fabsf(z0) + zspan + vl;
    const float S = fmaxf(fmaxf(fabsf(r0.x) * ax + fabsf(r0.y) * ay + fabsf(r0.z) * az + fabsf(r0.w),
                                fabsf(r1.x) * ax + fabsf(r1.y) * ay + fabsf(r1.z) * az + fabsf(r1.w)),
                          fabsf(r2.x) * ax + fabsf(r2.y) * ay + fabsf(r2.z) * az + fabsf(r2.w));
    const float eps = S * (1.0f / 262144.0f);
    const float bx = r0.x * xa + r0.y * ya + r0.z * z0 + r0.w, by = r1.x * xa + r1.y * ya + r1.z * z0 + r1.w,
                bz = r2.x * xa + r2.y * ya + r2.z * z0 + r2.w;
    const float dx[3] = {r0.x * (xb - xa), r0.y * (yb - ya), r0.z * zspan};
    const float dy[3] = {r1.x * (xb - xa), r1.y * (yb - ya), r1.z * zspan};
    const float dz[3] = {r2.x * (xb - xa), r2.y * (yb - ya), r2.z * zspan};
    float cx[8], cy[8], cz[8], zmin = bz;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        cx[c] = bx + ((c & 1) ? dx[0] : 0.0f) + ((c & 2) ? dx[1] : 0.0f) + ((c & 4) ? dx[2] : 0.0f);
        cy[c] = by + ((c & 1) ? dy[0] : 0.0f) + ((c & 2) ? dy[1] : 0.0f) + ((c & 4) ? dy[2] : 0.0f);
        cz[c] = bz + ((c & 1) ? dz[0] : 0.0f) + ((c & 2) ? dz[1] : 0.0f) + ((c & 4) ? dz[2] : 0.0f);
        zmin = fminf(zmin, cz[c]);
    }
    const float zl = zmin - eps;
    if (!(zl > 0.0f)) return true;   // a corner at or behind the camera plane (or a NaN)
    float umin = 3e38f, umax = -3e38f, vmin = 3e38f, vmax = -3e38f, mag = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float rz = gs2m_fast_rcp(cz[c]);                      // 1 ulp: within rnd below
        const float u = cx[c] * f0.fx_f * rz, v = cy[c] * f0.fy_f * rz;   // relative to the principal point
        umin = fminf(umin, u);
        umax = fmaxf(umax, u);
        vmin = fminf(vmin, v);
        vmax = fmaxf(vmax, v);
        mag += fabsf(u) + fabsf(v);   // fminf / fmaxf drop a NaN: this keeps it
    }
    if (!(mag < 1e9f)) return true;
    const float au = fmaxf(fabsf(umin), fabsf(umax)), av = fmaxf(fabsf(vmin), fabsf(vmax));
    const float k = eps / zl, rnd = 1.0f / 1048576.0f;
    const float mu = 1.0f + k * (fabsf(f0.fx_f) + au) + rnd * (au + fabsf(f0.cx_f) + 1.0f);
    const float mv = 1.0f + k * (fabsf(f0.fy_f) + av) + rnd * (av + fabsf(f0.cy_f) + 1.0f);
    if (!(mu < 1e6f && mv < 1e6f)) return true;
    const float x0 = fmaxf(floorf(umin + f0.cx_f - mu), 0.0f), x1 = fminf(ceilf(umax + f0.cx_f + mu), (float)(f0.W - 1));
    const float y0 = fmaxf(floorf(vmin + f0.cy_f - mv), 0.0f), y1 = fminf(ceilf(vmax + f0.cy_f + mv), (float)(f0.H - 1));
    if (x0 > x1 || y0 > y1) return false;   // no voxel sees a pixel.  Otherwise 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H
    const int tx0 = (int)x0 / GS2M_TSDF_TILE, tx1 = (int)x1 / GS2M_TSDF_TILE, ty0 = (int)y0 / GS2M_TSDF_TILE, ty1 = (int)y1 / GS2M_TSDF_TILE;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > GS2M_TSDF_CULL_MAX_TILES) return true;   // a camera this close: not worth the reads
    // 4 x 4 tiles per round trip: a tile past the footprint's edge reads the edge tile again (harmless to a maximum), so the
    // 16 loads are unconditional and go out together.  A micro-column's footprint is 2-4 tiles wide and up to 9 long.
    float dmax = 0.0f;
    for (int ty = ty0; ty <= ty1; ty += 4) {
        for (int tx = tx0; tx <= tx1; tx += 4) {
            float d[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* __restrict__ row = tiles + (size_t)(ty + i < ty1 ? ty + i : ty1) * tiles_x;
#pragma unroll
                for (int j = 0; j < 4; ++j) d[4 * i + j] = row[tx + j < tx1 ? tx + j : tx1];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (d[i] > dmax) dmax = d[i];
        }
    }
    if (!(dmax > 0.0f)) return false;   // no depth sample in the footprint
    const float zlow = zl - vl;
    return !(dmax - zlow <= -f0.sdf_trunc_f);
}

GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_integrate_batch(TsdfVolume V, const TsdfBatchFrame* __restrict__ frames, const float* __restrict__ tiles) {
    __shared__ float s_p0[16], s_p1[16];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lz = lane >> 4, lx = (lane >> 2) & 3, ly = lane & 3;
    __shared__ unsigned s_it;
    const unsigned n_touched = V.counters[1] * 4u;   // work items: (block, x-quarter)
    const TsdfFrame& f0 = frames[0].f;   // volume constants (voxel length, truncation) are the same in every frame
    for (;;) {
        // blocks are handed out dynamically (counters[3], zeroed before the launch): a block costs as many frame passes as
        // frames touched it (1 ... the batch size), so a static round-robin leaves the workgroups 1.5x apart at the end
        __syncthreads();  // previous block's readers of s_p0 / s_p1 / s_it (and of fmask) are done
        if (tid == 0) s_it = atomicAdd(&V.counters[3], 1u);
        __syncthreads();
        const unsigned it = s_it;
        if (it >= n_touched) break;
        const int xq = (int)(it & 3u);
        const unsigned h = V.touched[it >> 2];
        const unsigned long long key = V.hash_keys[h];
        const int slot = V.hash_vals[h];
        const unsigned long long fm = V.fmask[h];
        if (slot < 0) continue;   // pool overflow (flagged); uniform across the workgroup
        const float p2 = tsdf_block_centres(f0, key, tid, s_p0, s_p1);
        __syncthreads();
        const float p0 = s_p0[4 * xq + lx], p1 = s_p1[4 * wave + ly];
        const int vi0 = (xq * 4 + wave) * 64 + lane;   // = GS2M_TSDF_VINDEX(x, y, lz); the thread's voxel j (z = 4 j + lz) sits at vi0 + VS * j
        constexpr int VS = 16 * 64;                    // one micro-block layer of the block
        float* bt = V.tsdf + (size_t)slot * GS2M_TSDF_VOX;
        float* bw = V.weight + (size_t)slot * GS2M_TSDF_VOX;
        unsigned* bc = V.rgb + (size_t)slot * 3 * GS2M_TSDF_VOX;
        // The cull: lane f tests frame f of the batch (at most 64 of either) for THIS wave's micro-column, and the wave walks
        // only the frames the test could not prove dead.  The frame loop has no workgroup barrier, so the four waves may walk
        // different frame sets; a wave left without a frame skips its state loads and stores as well.
        bool live = false;
        if ((fm >> lane) & 1ull) {
            const int tiles_x = GS2M_TSDF_TILES(f0.W), tiles_y = GS2M_TSDF_TILES(f0.H);
            live = tsdf_pass_live(f0, reinterpret_cast<const float4*>(frames[lane].f.E), tiles + (size_t)lane * tiles_y * tiles_x, tiles_x,
                                  s_p0[4 * xq], s_p0[4 * xq + 3], s_p1[4 * wave], s_p1[4 * wave + 3], p2);
        }
        const unsigned long long fm_live = fm & gs2m_ballot(live ? 1 : 0);
        float w[4], t[4];
        unsigned c0[4], c1[4], c2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = t[j] = 0.0f;
            c0[j] = c1[j] = c2[j] = 0u;
            if (fm_live != 0ull) {
                w[j] = bw[vi0 + VS * j];
                t[j] = bt[vi0 + VS * j];
                if (V.has_color) {
                    c0[j] = bc[vi0 + VS * j];
                    c1[j] = bc[GS2M_TSDF_VOX + vi0 + VS * j];
                    c2[j] = bc[2 * GS2M_TSDF_VOX + vi0 + VS * j];
                }
            }
        }
        // Software pipeline over the frames of the block: the projection of frame n + 1 and its depth gathers are issued
        // before frame n is applied, so a wave always has the next frame's memory round trip in flight (the kernel is bound
        // by gather latency: 63 % of the wave cycles wait at 4 waves per SIMD, PMC).  Frames are still APPLIED in ascending
        // order with the same arithmetic: bit-identical to the frame-by-frame path.
        // What a probe keeps until it is applied is 9 registers (with 17 the kernel stood at 92 VGPRs = 5 waves per SIMD, now 74 = 6).
        struct Probe {
            int fi;
            unsigned uv[4];        // u | v << 16 (image sizes <= 65535, checked by the host side), or NO_PIXEL
            float zc0;             // camera-space z of the thread's first voxel: apply() repeats the chain's additions on it
            float d[4];
        };
        constexpr unsigned NO_PIXEL = 0xffffffffu;   // u, v <= 65534: no pixel packs to this
        auto probe = [&](const int fi, Probe& P) __attribute__((always_inline)) {
            const TsdfBatchFrame& bf = frames[fi];
            const TsdfFrame& f = bf.f;
            const float* __restrict__ depth = bf.depth;
            const unsigned char* __restrict__ mask = bf.mask;
            P.fi = fi;
            // camera-space centre of voxel (x, y, 0), advanced along z to the thread's first voxel (x, y, lz)
            float pc0, pc1, pc2;
            tsdf_cam_point(f, p0, p1, p2, pc0, pc1, pc2);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (s < lz) tsdf_z_step(f, pc0, pc1, pc2);
            }
            P.zc0 = pc2;
            int pix[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int u = 0, v = 0;
                pix[j] = tsdf_project(f, pc0, pc1, pc2, u, v);
                P.uv[j] = pix[j] >= 0 ? ((unsigned)u | ((unsigned)v << 16)) : NO_PIXEL;
#pragma unroll
                for (int s = 0; s < 4; ++s) tsdf_z_step(f, pc0, pc1, pc2);   // to the same position in the next micro-block
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)   // depth gathers, back to back (converted and consumed by apply() one frame later)
                P.d[j] = pix[j] >= 0 ? tsdf_read_depth(f, depth, mask, (size_t)pix[j]) : 0.0f;
        };
        auto apply = [&](Probe& P) __attribute__((always_inline)) {
            const TsdfBatchFrame& bf = frames[P.fi];
            const TsdfFrame& f = bf.f;
            const unsigned char* __restrict__ color = bf.color;
            const int last_pix = f.W * f.H - 1;
            unsigned rgbp[4];
            bool upd[4];
            float tnew[4];
            float zx = 0.0f, zy = 0.0f, zc = P.zc0;   // the z chain again, of which only z is used
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                upd[j] = false;
                tnew[j] = 0.0f;
                rgbp[j] = 0u;
                const bool seen = P.uv[j] != NO_PIXEL;
                const float zcj = zc;
#pragma unroll
                for (int s = 0; s < 4; ++s) tsdf_z_step(f, zx, zy, zc);
                // (measured, profiles/tsdf_update_once.txt: leaving the iteration early where pix < 0 instead of these two
                // guards costs the sweep 3 % -- 28.69 / 28.95 / 29.00 against 27.97 / 28.05 / 27.88 us per frame, C2 in sweeps
                // of 20, runs interleaved in one session -- same arithmetic, another schedule)
                float dd = P.d[j];
                if (seen) dd = tsdf_convert_depth(f, dd);
                if (seen && dd > 0.0f) {
                    // the distance multiplier (a correctly rounded sqrt) only here, where a depth sample exists
                    const int u = (int)(P.uv[j] & 0xffffu), v = (int)(P.uv[j] >> 16);
                    const float mult = tsdf_distance_multiplier(f, u, v);
                    upd[j] = tsdf_decide(f, dd, zcj, mult, tnew[j]);
                    if (upd[j] && V.has_color) rgbp[j] = tsdf_gather_rgb(color, v * f.W + u, last_pix);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (upd[j]) {
                    tsdf_update_mean(t[j], w[j], tnew[j]);
                    tsdf_update_rgb(c0[j], c1[j], c2[j], rgbp[j]);   // rgbp = 0 and sums of 0 in a volume without colour
                }
            }
        };
        unsigned long long todo = fm_live;
        Probe A, B;
        if (todo != 0ull) {
            probe(__ffsll(todo) - 1, A);   // frames in ascending order
            todo &= todo - 1ull;
            while (todo != 0ull) {
                probe(__ffsll(todo) - 1, B);
                todo &= todo - 1ull;
                apply(A);
                if (todo == 0ull) {
                    A = B;
                    break;
                }
                probe(__ffsll(todo) - 1, A);
                todo &= todo - 1ull;
                apply(B);
                if (todo == 0ull) break;
            }
            apply(A);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (fm_live == 0ull) continue;   // nothing loaded, nothing changed
            bw[vi0 + VS * j] = w[j];
            bt[vi0 + VS * j] = t[j];
            if (V.has_color) {
                bc[vi0 + VS * j] = c0[j];
                bc[GS2M_TSDF_VOX + vi0 + VS * j] = c1[j];
                bc[2 * GS2M_TSDF_VOX + vi0 + VS * j] = c2[j];
            }
        }
        if (tid == 0 && xq == 0) atomicAdd(&V.totals[0], (unsigned long long)gs2m_popc64(fm));   // block updates = sum over frames of touched blocks
    }
}

// after k_tsdf_integrate_batch: frame masks of the touched blocks back to 0 for the next batch
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_clear_fmask(TsdfVolume V) {
    const unsigned n = V.counters[1];
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) V.fmask[V.touched[i]] = 0ull;
}

// Reset without touching the unused part of the pool: blocks are handed out in slot order, so only slots
// [0, counters[0]) can hold state (a dense 512^3 pool is 2.7 GB; a scan touches a few hundred MB of it).
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_clear_used(TsdfVolume V) {
    unsigned n = V.counters[0];
    if (n > V.max_blocks) n = V.max_blocks;
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (unsigned slot = blockIdx.x; slot < n; slot += gridDim.x) {
        float4* t4 = reinterpret_cast<float4*>(V.tsdf + (size_t)slot * GS2M_TSDF_VOX);
        float4* w4 = reinterpret_cast<float4*>(V.weight + (size_t)slot * GS2M_TSDF_VOX);
        for (int i = (int)threadIdx.x; i < GS2M_TSDF_VOX / 4; i += 256) {
            t4[i] = z;
            w4[i] = z;
        }
        if (V.has_color) {
            float4* c4 = reinterpret_cast<float4*>(V.rgb + (size_t)slot * 3 * GS2M_TSDF_VOX);
            for (int i = (int)threadIdx.x; i < 3 * GS2M_TSDF_VOX / 4; i += 256) c4[i] = z;
        }
        if (threadIdx.x == 0) V.halo[slot] = 0;
    }
}

// gs2m_tsdf_replace: the slots [first, counters[0]) back to the clean state (the blocks about to be unpacked overwrite slots
// [0, first) completely: clearing those as well -- what a reset does -- would write the reduced volume's bytes twice)
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_clear_from(TsdfVolume V, unsigned first) {
    unsigned n = V.counters[0];
    if (n > V.max_blocks) n = V.max_blocks;
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (unsigned slot = first + blockIdx.x; slot < n; slot += gridDim.x) {
        float4* t4 = reinterpret_cast<float4*>(V.tsdf + (size_t)slot * GS2M_TSDF_VOX);
        float4* w4 = reinterpret_cast<float4*>(V.weight + (size_t)slot * GS2M_TSDF_VOX);
        for (int i = (int)threadIdx.x; i < GS2M_TSDF_VOX / 4; i += 256) {
            t4[i] = z;
            w4[i] = z;
        }
        if (V.has_color) {
            float4* c4 = reinterpret_cast<float4*>(V.rgb + (size_t)slot * 3 * GS2M_TSDF_VOX);
            for (int i = (int)threadIdx.x; i < 3 * GS2M_TSDF_VOX / 4; i += 256) c4[i] = z;
        }
        if (threadIdx.x == 0) V.halo[slot] = 0;
    }
}

// gs2m_tsdf_replace, after its unpack: the unpack hands out slots [0, counters[0]) -- exactly [0, upto) for `upto` distinct in-range
// keys, fewer when a key repeats, lies outside the key range or the hash table is full.  The slots it did NOT hand out,
// [counters[0], upto), were skipped by k_tsdf_clear_from and still hold the previous volume's state: cleared here, on the device,
// so that stale voxels never reappear in a block allocated later.  No work in the regular case (counters[0] == upto).
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_clear_gap(TsdfVolume V, unsigned upto) {
    unsigned first = V.counters[0];
    if (upto > V.max_blocks) upto = V.max_blocks;
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (unsigned slot = first + blockIdx.x; slot < upto; slot += gridDim.x) {
        float4* t4 = reinterpret_cast<float4*>(V.tsdf + (size_t)slot * GS2M_TSDF_VOX);
        float4* w4 = reinterpret_cast<float4*>(V.weight + (size_t)slot * GS2M_TSDF_VOX);
        for (int i = (int)threadIdx.x; i < GS2M_TSDF_VOX / 4; i += 256) {
            t4[i] = z;
            w4[i] = z;
        }
        if (V.has_color) {
            float4* c4 = reinterpret_cast<float4*>(V.rgb + (size_t)slot * 3 * GS2M_TSDF_VOX);
            for (int i = (int)threadIdx.x; i < 3 * GS2M_TSDF_VOX / 4; i += 256) c4[i] = z;
        }
        if (threadIdx.x == 0) V.halo[slot] = 0;
    }
}

// ---- multi-GPU exchange -----------------------------------------------------------------------
// Exchange forms (GS2M_XFORM_*, include/gs2mesh_amd.h):
//   0 SUM_F32     one fp32 buffer [n][5][4096]: planes wsum = tsdf * weight, weight, sum r, sum g, sum b -- counts and colour
//                 sums are integers < 2^24, exact in fp32 and independent of the reduction order (one fp32 SUM collective);
//   1 RAW_F32     the same buffer with the planes VERBATIM (tsdf, weight, sums): for blocks that are already reduced
//                 (halo copies: fl(fl(t * w) / w) is not always t);
//   2 SUM_PACKED  wsum as fp32 [n][4096] + ONE int64 per voxel  w | sum r << 10 | sum g << 28 | sum b << 46  (valid while the
//                 volume has seen <= 1023 frames: w < 2^10, colour sums <= 255 * 1023 < 2^18, no carry between the fields
//                 under an integer SUM): 12 instead of 20 bytes per voxel on the wire.
// pack: one workgroup per canonical key (zeros where the block is not allocated here or only a halo copy).
#define GS2M_XF_SUM_F32 0
#define GS2M_XF_RAW_F32 1
#define GS2M_XF_SUM_PACKED 2
template <int FORM>
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_pack(TsdfVolume V, const int* __restrict__ keys, float* __restrict__ buf, long long* __restrict__ ibuf) {
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    const int bx = keys[3 * b], by = keys[3 * b + 1], bz = keys[3 * b + 2];
    int slot = tsdf_key_in_range(bx, by, bz) ? tsdf_lookup(V, tsdf_pack_key(bx, by, bz)) : -1;
    if (slot >= 0 && FORM != GS2M_XF_RAW_F32 && V.halo[slot]) slot = -1;   // a halo copy is another rank's block: never summed twice
    float* o = buf + b * (FORM == GS2M_XF_SUM_PACKED ? 1 : 5) * GS2M_TSDF_VOX;
    for (int i = tid; i < GS2M_TSDF_VOX; i += 256) {
        float w = 0.f, t = 0.f;
        unsigned c0 = 0u, c1 = 0u, c2 = 0u;
        if (slot >= 0) {
            w = V.weight[(size_t)slot * GS2M_TSDF_VOX + i];
            t = V.tsdf[(size_t)slot * GS2M_TSDF_VOX + i];
            if (FORM != GS2M_XF_RAW_F32) t = t * w;
            if (V.has_color) {
                c0 = V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + i];
                c1 = V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + GS2M_TSDF_VOX + i];
                c2 = V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + 2 * GS2M_TSDF_VOX + i];
            }
        }
        o[i] = t;
        if (FORM == GS2M_XF_SUM_PACKED) {
            // the fields only stay apart under an integer SUM while w < 2^10 and the colour sums < 2^18 IN THE RESULT; a
            // local value that already exceeds its field is flagged (status bit 8): the caller's frame bound was wrong
            // (state injected through unpack, C-API users) -- checked by gs2mesh_amd.parallel after the exchange
            if (w > 1023.0f || ((c0 | c1 | c2) >> 18) != 0u) atomicOr(&V.counters[2], 8u);
            ibuf[b * GS2M_TSDF_VOX + i] = (long long)((unsigned long long)(unsigned)w | ((unsigned long long)c0 << 10) |
                                                      ((unsigned long long)c1 << 28) | ((unsigned long long)c2 << 46));
        } else {
            o[GS2M_TSDF_VOX + i] = w;
            o[2 * GS2M_TSDF_VOX + i] = (float)c0;
            o[3 * GS2M_TSDF_VOX + i] = (float)c1;
            o[4 * GS2M_TSDF_VOX + i] = (float)c2;
        }
    }
}

// unpack: replaces the state of the listed blocks (allocating as needed): tsdf = wsum / weight (SUM forms) or verbatim
// (RAW); `halo` marks them as neighbour-only blocks of another rank's part of the volume (mesh extraction reads them but
// starts no cube there; pack / block_keys skip them).
template <int FORM>
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_unpack(TsdfVolume V, const int* __restrict__ keys, const float* __restrict__ buf, const long long* __restrict__ ibuf,
              int halo) {
    __shared__ int s_slot;
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    if (tid == 0) {
        const int bx = keys[3 * b], by = keys[3 * b + 1], bz = keys[3 * b + 2];
        int slot = -1;
        if (tsdf_key_in_range(bx, by, bz)) {
            const unsigned h = tsdf_find_or_insert(V, tsdf_pack_key(bx, by, bz), bx, by, bz);
            if (h != 0xffffffffu) slot = V.hash_vals[h];
        } else {
            atomicOr(&V.counters[2], 4u);
        }
        if (slot >= 0) V.halo[slot] = (unsigned char)(halo ? 1 : 0);
        s_slot = slot;
    }
    __syncthreads();
    const int slot = s_slot;
    if (slot < 0) return;
    const float* in = buf + b * (FORM == GS2M_XF_SUM_PACKED ? 1 : 5) * GS2M_TSDF_VOX;
    for (int i = tid; i < GS2M_TSDF_VOX; i += 256) {
        float w;
        unsigned c0, c1, c2;
        if (FORM == GS2M_XF_SUM_PACKED) {
            const unsigned long long p = (unsigned long long)ibuf[b * GS2M_TSDF_VOX + i];
            w = (float)(unsigned)(p & 0x3ffull);
            c0 = (unsigned)((p >> 10) & 0x3ffffull);
            c1 = (unsigned)((p >> 28) & 0x3ffffull);
            c2 = (unsigned)(p >> 46);
        } else {
            w = in[GS2M_TSDF_VOX + i];
            c0 = (unsigned)in[2 * GS2M_TSDF_VOX + i];
            c1 = (unsigned)in[3 * GS2M_TSDF_VOX + i];
            c2 = (unsigned)in[4 * GS2M_TSDF_VOX + i];
        }
        V.weight[(size_t)slot * GS2M_TSDF_VOX + i] = w;
        V.tsdf[(size_t)slot * GS2M_TSDF_VOX + i] = FORM == GS2M_XF_RAW_F32 ? in[i] : (w > 0.f ? in[i] / w : 0.f);
        if (V.has_color) {
            V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + i] = c0;
            V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + GS2M_TSDF_VOX + i] = c1;
            V.rgb[(size_t)slot * 3 * GS2M_TSDF_VOX + 2 * GS2M_TSDF_VOX + i] = c2;
        }
    }
}

// block keys of the first n slots; halo copies (another rank's blocks) are reported as the out-of-range sentinel key
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_owned_keys(TsdfVolume V, unsigned n, int* __restrict__ keys) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const bool h = V.halo[s] != 0;
    const int sentinel = GS2M_TSDF_KEY_BIAS - 1;
    keys[3 * (size_t)s] = h ? sentinel : V.block_keys[3 * (size_t)s];
    keys[3 * (size_t)s + 1] = h ? sentinel : V.block_keys[3 * (size_t)s + 1];
    keys[3 * (size_t)s + 2] = h ? sentinel : V.block_keys[3 * (size_t)s + 2];
}

// ---- block-map key exchange (round 5) -----------------------------------------------------------
// The union of the ranks' block sets is formed as a dense MAP over a window of block indices: every rank marks its own blocks,
// ONE all_reduce merges the ranks, and the canonical key list is the marked cells in cell order -- identical on every rank, no
// gather, no sort, no host pass over keys.  SURVEY 8e asks for a bitmap under a bitwise OR; RCCL (like NCCL) has no bitwise
// reduction, so the map holds one BYTE per block and the collective is MAX over uint8 (32 KiB for a 32^3-block window, 256 KiB
// for the default 64^3).  Window: lo[k] <= b[k] < lo[k] + dim[k];
//   cell = ((bx - lo.x) * dim.y + (by - lo.y)) * dim.z + (bz - lo.z)     (ascending cell = ascending (x, y, z) = packed-key order)
// The header travels behind the map in the same buffer (GS2M_TSDF_MAP_HEADER bytes + 8 per rank), arranged so that a bytewise MAX
// reduces it: flags are 0 / 1 bytes; values that must agree are sent as the bytes of x and of ~x (byte + complement byte == 255
// after the MAX <=> all ranks sent the same byte); every rank writes its frame counts into its OWN slot (the others send zeros).
//   [0] a block outside the window (every rank then takes the gather path)     [1..4] overflow flags 1, 2, 4, 8 of V.counters[2]
//   [5] replicated   [6] holds halo copies   [8..11] / [12..15] max_blocks / ~max_blocks   [16..19] / [20..23] window hash / ~hash
//   [24..27] number of marked cells (written by k_tsdf_map_keys on the reduced buffer)
//   [32 + 8 r .. +3] frames_local, [36 + 8 r .. +3] frames_base of rank r (little endian)
#define GS2M_TSDF_MAP_HEADER 32
GS2M_DEVICE void tsdf_put_u32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)(v & 255u);
    p[1] = (unsigned char)((v >> 8) & 255u);
    p[2] = (unsigned char)((v >> 16) & 255u);
    p[3] = (unsigned char)(v >> 24);
}
GS2M_KERNEL void __launch_bounds__(256)
k_tsdf_block_map(TsdfVolume V, int lox, int loy, int loz, int dx, int dy, int dz, unsigned char* __restrict__ cells, unsigned n_cells,
                 unsigned flags, unsigned win_hash, int rank, unsigned frames_local, unsigned frames_base) {
    unsigned n = V.counters[0];
    if (n > V.max_blocks) n = V.max_blocks;
    unsigned char* hdr = cells + n_cells;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned ov = V.counters[2];
        for (int b = 0; b < 4; ++b) hdr[1 + b] = (unsigned char)((ov >> b) & 1u);
        hdr[5] = (unsigned char)(flags & 1u);
        hdr[6] = (unsigned char)((flags >> 1) & 1u);
        tsdf_put_u32(hdr + 8, V.max_blocks);
        tsdf_put_u32(hdr + 12, ~V.max_blocks);
        tsdf_put_u32(hdr + 16, win_hash);
        tsdf_put_u32(hdr + 20, ~win_hash);
        tsdf_put_u32(hdr + GS2M_TSDF_MAP_HEADER + 8 * rank, frames_local);
        tsdf_put_u32(hdr + GS2M_TSDF_MAP_HEADER + 8 * rank + 4, frames_base);
    }
    for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < n; s += gridDim.x * 256u) {
        if (V.halo[s]) continue;     // a halo copy is another rank's block
        const int bx = V.block_keys[3 * (size_t)s] - lox, by = V.block_keys[3 * (size_t)s + 1] - loy, bz = V.block_keys[3 * (size_t)s + 2] - loz;
        if (bx < 0 || by < 0 || bz < 0 || bx >= dx || by >= dy || bz >= dz) {
            hdr[0] = 1;
            continue;
        }
        cells[((size_t)bx * (unsigned)dy + (unsigned)by) * (unsigned)dz + (unsigned)bz] = 1;
    }
}

// Marked cells of the (reduced) map -> keys [n][3] in cell order; header bytes [24..27] = n.  One 1024-thread workgroup: thread t
// owns the consecutive cells [t * per, (t + 1) * per), per a multiple of 16 (16-byte loads): count, workgroup exclusive scan,
// emit.  Keys beyond max_keys are counted, not written (the caller compares n with its buffer).
GS2M_KERNEL void __launch_bounds__(1024)
k_tsdf_map_keys(int lox, int loy, int loz, int dy, int dz, unsigned char* __restrict__ cells, unsigned n_cells, int* __restrict__ keys,
                unsigned max_keys) {
    __shared__ unsigned wave_sum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned per = ((n_cells + 1023u) / 1024u + 15u) & ~15u;
    const unsigned c0 = (unsigned)tid * per < n_cells ? (unsigned)tid * per : n_cells;
    const unsigned c1 = c0 + per < n_cells ? c0 + per : n_cells;
    unsigned cnt = 0;
    for (unsigned c = c0; c < c1; c += 16u) {
        if (c + 16u <= c1) {
            const uint4 v = *reinterpret_cast<const uint4*>(cells + c);      // the buffer is 16-byte aligned, c0 a multiple of 16
            // cells are 0 / 1 bytes: the byte sum of a word = its number of marked cells
            const unsigned t = (v.x & 0x01010101u) + (v.y & 0x01010101u) + (v.z & 0x01010101u) + (v.w & 0x01010101u);
            cnt += (t & 255u) + ((t >> 8) & 255u) + ((t >> 16) & 255u) + (t >> 24);
        } else {
            for (unsigned k = c; k < c1; ++k) cnt += cells[k] ? 1u : 0u;
        }
    }
    unsigned inc = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = gs2m_shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int k = 0; k < wave; ++k) base += wave_sum[k];
    unsigned pos = base + inc - cnt;
    if (tid == 1023) tsdf_put_u32(cells + n_cells + 24, base + inc);
    if (cnt == 0u) return;
    for (unsigned c = c0; c < c1; ++c) {
        if (!cells[c]) continue;
        if (pos < max_keys) {
            const unsigned z = c % (unsigned)dz, xy = c / (unsigned)dz;
            keys[3 * (size_t)pos] = (int)(xy / (unsigned)dy) + lox;
            keys[3 * (size_t)pos + 1] = (int)(xy % (unsigned)dy) + loy;
            keys[3 * (size_t)pos + 2] = (int)z + loz;
        }
        ++pos;
    }
}
