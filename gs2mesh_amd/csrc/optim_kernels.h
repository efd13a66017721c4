// optim_kernels.h -- gs2m_adam_step / gs2m_densify_stats: the update phase of a 3DGS training iteration, two launches
// instead of torch.optim.Adam's chain of element-wise launches over six parameter groups and the boolean-mask reads and
// writes of the densification statistics (GS/train.py:113-127, GS/scene/gaussian_model.py:405-407).
//
// k_adam_multi: the Adam step of up to ADAM_MAX_SEGMENTS contiguous f32 tensors ("segments": parameter, gradient, two
// moments, own scalars) in ONE launch.
//   Table.   The segment table is the kernel argument, by value (AdamTable, 616 bytes of the kernarg segment): there is no
//            device-side table and no host-to-device copy, so the call is asynchronous on its stream and needs no scratch.
//   Layout.  One workgroup of ADAM_THREADS = 256 lanes owns ADAM_WG_ELEMS = 1024 consecutive elements of one segment; a lane
//            owns 4 consecutive elements.  Every segment starts on a workgroup boundary: first_wg[s] is the first workgroup of
//            segment s (unused entries 0xffffffff), and a workgroup finds its segment by counting the entries that are not
//            above its index -- at most 7 scalar compares, wave-uniform.  Element offsets are 64-bit.
//   Access.  Where the four pointers of a segment are 16-byte aligned (`vec`) a lane with four live elements moves each
//            array as one 16-byte load / store; the count % 4 tail, lanes that are only partly visible and segments that are
//            not aligned go element by element.  One lane owns each element, no atomics, in place: the same bits every run.
//   Sparse.  With row_visible (int32 per row; visible where > 0) element e of a segment of row width w belongs to row
//            e / w.  A lane reads the visibility of its (at most four) rows first; elements of invisible rows are neither
//            read nor written, and a lane with nothing visible issues no load of p, g, m or v.
//
// Arithmetic (include/gs2mesh_amd.h states it; tests/adam_statement.py restates it in numpy).  This header is compiled into
// train_kernels.hip, built with -ffp-contract=off: every operation is one f32 operation rounded on its own, the division
// and the square root are the IEEE ones, subnormals are kept, parentheses are the order.  The six scalars come from the
// host, computed in double and cast to f32 last (adam_scalars):
//   ss = f32(lr / (1 - beta1^t)), bs = f32(sqrt(1 - beta2^t)), omb1 = f32(1 - beta1), b2 = f32(beta2), omb2 = f32(1 - beta2)
//   m' = m + omb1 * (g - m)
//   v' = b2 * v + (omb2 * g) * g
//   p' = p - ss * (m' / (sqrt(v') / bs + f32(eps)))
//
// k_densify_stats: one Gaussian per lane; where radii[i] > 0
//   r = (float)radii[i];  max_radii2D[i] = r > max_radii2D[i] ? r : max_radii2D[i]
//   n = sqrt(gx * gx + gy * gy)  (columns 0 and 1 of the [P,3] viewspace gradient);  grad_accum[i] += n;  denom[i] += 1
#pragma once

#define ADAM_MAX_SEGMENTS 8
#define ADAM_THREADS 256
#define ADAM_LANE_ELEMS 4
#define ADAM_WG_ELEMS (ADAM_THREADS * ADAM_LANE_ELEMS)
#define ADAM_NO_WG 0xffffffffu

struct AdamSegment {                      // 72 bytes
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t count;
    int row_width;
    int vec;                              // the four pointers are 16-byte aligned
    float ss, bs, omb1, b2, omb2, eps;
};

struct AdamTable {
    AdamSegment seg[ADAM_MAX_SEGMENTS];
    unsigned first_wg[ADAM_MAX_SEGMENTS + 1];     // [n] = the grid; ADAM_NO_WG past it
    int n;
};

// the scalars of one segment, in double, cast last
static inline void adam_scalars(AdamSegment& s, double lr, double beta1, double beta2, double eps, int64_t step) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    s.ss = (float)(lr / bc1);
    s.bs = (float)sqrt(bc2);
    s.omb1 = (float)(1.0 - beta1);
    s.b2 = (float)beta2;
    s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
}

GS2M_DEVICE void adam_element(float& p, float g, float& m, float& v, float ss, float bs, float omb1, float b2, float omb2,
                              float eps) {
    m = m + omb1 * (g - m);
    v = b2 * v + (omb2 * g) * g;
    p = p - ss * (m / (sqrtf(v) / bs + eps));
}

GS2M_KERNEL void __launch_bounds__(ADAM_THREADS)
k_adam_multi(AdamTable T, const int* __restrict__ row_visible) {
    const unsigned wg = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MAX_SEGMENTS; ++k) s += wg >= T.first_wg[k] ? 1 : 0;   // first_wg ascends; ADAM_NO_WG never counts
    const AdamSegment& S = T.seg[s];
    const int64_t count = S.count;
    const int64_t e0 = (int64_t)(wg - T.first_wg[s]) * ADAM_WG_ELEMS + (int64_t)threadIdx.x * ADAM_LANE_ELEMS;
    if (e0 >= count) return;
    const int n = count - e0 < ADAM_LANE_ELEMS ? (int)(count - e0) : ADAM_LANE_ELEMS;
    unsigned mask = (1u << n) - 1u;
    if (row_visible) {
        const int w = S.row_width;
        int64_t row;
        int rem;
        if (count <= 0x7fffffffll) {          // wave-uniform: the 32-bit division where it is enough
            const unsigned e = (unsigned)e0;
            row = (int64_t)(e / (unsigned)w);
            rem = (int)(e % (unsigned)w);
        } else {
            row = e0 / w;
            rem = (int)(e0 % w);
        }
        bool visible = row_visible[row] > 0;
        mask = 0u;
        for (int k = 0; k < n; ++k) {
            mask |= (visible ? 1u : 0u) << k;
            if (++rem == w && k + 1 < n) {      // element e0 + k + 1 < count = rows * w: its row exists
                rem = 0;
                ++row;
                visible = row_visible[row] > 0;
            }
        }
        if (mask == 0u) return;
    }
    const float ss = S.ss, bs = S.bs, omb1 = S.omb1, b2 = S.b2, omb2 = S.omb2, eps = S.eps;
    float* __restrict__ p = S.p + e0;
    const float* __restrict__ g = S.g + e0;
    float* __restrict__ m = S.m + e0;
    float* __restrict__ v = S.v + e0;
    if (mask == 15u && S.vec) {
        float4 p4 = *reinterpret_cast<const float4*>(p);
        const float4 g4 = *reinterpret_cast<const float4*>(g);
        float4 m4 = *reinterpret_cast<const float4*>(m), v4 = *reinterpret_cast<const float4*>(v);
        adam_element(p4.x, g4.x, m4.x, v4.x, ss, bs, omb1, b2, omb2, eps);
        adam_element(p4.y, g4.y, m4.y, v4.y, ss, bs, omb1, b2, omb2, eps);
        adam_element(p4.z, g4.z, m4.z, v4.z, ss, bs, omb1, b2, omb2, eps);
        adam_element(p4.w, g4.w, m4.w, v4.w, ss, bs, omb1, b2, omb2, eps);
        *reinterpret_cast<float4*>(p) = p4;
        *reinterpret_cast<float4*>(m) = m4;
        *reinterpret_cast<float4*>(v) = v4;
        return;
    }
    for (int k = 0; k < ADAM_LANE_ELEMS; ++k) {
        if (!((mask >> k) & 1u)) continue;
        float pk = p[k], mk = m[k], vk = v[k];
        adam_element(pk, g[k], mk, vk, ss, bs, omb1, b2, omb2, eps);
        p[k] = pk;
        m[k] = mk;
        v[k] = vk;
    }
}

GS2M_KERNEL void __launch_bounds__(256)
k_densify_stats(int P, const int* __restrict__ radii, const float* __restrict__ viewspace_grad, float* __restrict__ max_radii2D,
                float* __restrict__ grad_accum, float* __restrict__ denom) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i >= P) return;
    const int radius = radii[i];
    if (radius <= 0) return;
    const float r = (float)radius, old = max_radii2D[i];
    max_radii2D[i] = r > old ? r : old;
    const float gx = viewspace_grad[3 * (size_t)i], gy = viewspace_grad[3 * (size_t)i + 1];
    grad_accum[i] = grad_accum[i] + sqrtf(gx * gx + gy * gy);
    denom[i] = denom[i] + 1.0f;
}
