// mesh_kernels.h -- device-side mesh post-processing of the fuse half:
//   * welding the marching-cubes triangle soup by Open3D's vertex identity (the cut edge: global voxel index of its lower corner
//     + axis; ScalableTSDFVolume::ExtractTriangleMesh keeps an edge -> vertex map) -- gs2mesh_utils/tsdf_utils.py:108;
//   * connected components over shared edges (TriangleMesh::ClusterConnectedTriangles) -- tsdf_utils.py:133.
// Both used to run on the host (numpy unique / scipy connected_components) on a 144 B-per-triangle soup copied over PCIe.
//
// Weld: an open-addressing hash table keyed by the 62-bit edge key keeps, per key, the SMALLEST soup index that carries it
// (atomicMin): the vertex order of the result is first appearance in the soup, which is what the host path produced and what makes
// the output independent of the arrival order of the threads.  An exclusive scan of the "I am the first" flags numbers the
// vertices; a last pass writes the compact arrays and the triangle indices.
// Cluster: lock-free union-find (hook the larger root under the smaller with atomicCAS, path halving).  A second hash table maps
// an undirected edge (vmin, vmax) to the first triangle that registered it; every other triangle with that edge is united with it.
// The root of a component is its smallest triangle index, so numbering the roots in index order reproduces the labels of a
// breadth-first sweep from triangle 0 upwards (scipy / Open3D number clusters by their first triangle).
#pragma once
#include "platform.h"

#define GS2M_MESH_EMPTY 0xffffffffffffffffull

GS2M_DEVICE unsigned mesh_hash64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

// find-or-insert `key` (never GS2M_MESH_EMPTY) -> cell index; cap is a power of two > the number of distinct keys
GS2M_DEVICE unsigned mesh_table_cell(unsigned long long* __restrict__ hkeys, unsigned cap, unsigned long long key) {
    const unsigned mask = cap - 1u;
    unsigned h = mesh_hash64(key) & mask;
    for (;;) {
        const unsigned long long k = hkeys[h];
        if (k == key) return h;
        if (k == GS2M_MESH_EMPTY) {
            const unsigned long long prev = atomicCAS(&hkeys[h], GS2M_MESH_EMPTY, key);
            if (prev == GS2M_MESH_EMPTY || prev == key) return h;
        }
        h = (h + 1u) & mask;
    }
}

// ---- weld ---------------------------------------------------------------------------------------------------------------
// per-axis minimum of the soup's voxel indices (the keys are made relative to it): mins[3] start at INT_MAX
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_key_min(const int* __restrict__ edge_index, unsigned n, int* __restrict__ mins) {
    __shared__ int s_min[3];
    if (threadIdx.x < 3) s_min[threadIdx.x] = 0x7fffffff;
    __syncthreads();
    int m0 = 0x7fffffff, m1 = 0x7fffffff, m2 = 0x7fffffff;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const int x = edge_index[4 * (size_t)i], y = edge_index[4 * (size_t)i + 1], z = edge_index[4 * (size_t)i + 2];
        m0 = x < m0 ? x : m0;
        m1 = y < m1 ? y : m1;
        m2 = z < m2 ? z : m2;
    }
    // one LDS atomic per thread, one global atomic per workgroup (every thread on the three global words: 0.56 ms for 2.6 M keys)
    atomicMin(&s_min[0], m0);
    atomicMin(&s_min[1], m1);
    atomicMin(&s_min[2], m2);
    __syncthreads();
    if (threadIdx.x < 3 && s_min[threadIdx.x] != 0x7fffffff) atomicMin(&mins[threadIdx.x], s_min[threadIdx.x]);
}

// 62-bit key of soup vertex i: 20 bits per axis relative to mins, 2 bits axis; bad[0] |= 1 if the soup spans more than 2^20 voxels
GS2M_DEVICE unsigned long long mesh_edge_key(const int* __restrict__ edge_index, size_t i, const int* __restrict__ mins, unsigned* bad) {
    const unsigned x = (unsigned)(edge_index[4 * i] - mins[0]), y = (unsigned)(edge_index[4 * i + 1] - mins[1]);
    const unsigned z = (unsigned)(edge_index[4 * i + 2] - mins[2]), a = (unsigned)edge_index[4 * i + 3];
    if ((x | y | z) >> 20 || a > 2u) atomicOr(bad, 1u);
    return (unsigned long long)(x & 0xfffffu) | ((unsigned long long)(y & 0xfffffu) << 20) | ((unsigned long long)(z & 0xfffffu) << 40) |
           ((unsigned long long)(a & 3u) << 60);
}

// pass 1: cell of every soup vertex; per cell the smallest soup index (hfirst starts at 0xffffffff)
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_weld_insert(const int* __restrict__ edge_index, unsigned n, const int* __restrict__ mins, unsigned long long* __restrict__ hkeys,
                   unsigned* __restrict__ hfirst, unsigned cap, unsigned* __restrict__ cell_of, unsigned* __restrict__ bad) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned c = mesh_table_cell(hkeys, cap, mesh_edge_key(edge_index, i, mins, bad));
        cell_of[i] = c;
        atomicMin(&hfirst[c], i);
    }
}
// pass 2: flag[i] = 1 where soup vertex i is the first carrier of its key
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_weld_flag(unsigned n, const unsigned* __restrict__ hfirst, const unsigned* __restrict__ cell_of, unsigned* __restrict__ flag) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) flag[i] = hfirst[cell_of[i]] == i ? 1u : 0u;
}
// pass 3 (after the exclusive scan of flag -> pos): triangle indices; the first carriers write the compact vertex arrays
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_weld_emit(unsigned n, const unsigned* __restrict__ hfirst, const unsigned* __restrict__ cell_of, const unsigned* __restrict__ pos,
                 const double* __restrict__ verts, const double* __restrict__ cols, const int* __restrict__ edge_index,
                 double* __restrict__ out_v, double* __restrict__ out_c, int* __restrict__ out_e, int* __restrict__ out_tri) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned f = hfirst[cell_of[i]];
        const unsigned p = pos[f];
        out_tri[i] = (int)p;
        if (f == i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                out_v[3 * (size_t)p + k] = verts[3 * (size_t)i + k];
                if (out_c) out_c[3 * (size_t)p + k] = cols ? cols[3 * (size_t)i + k] : 0.0;
            }
            if (out_e) {
#pragma unroll
                for (int k = 0; k < 4; ++k) out_e[4 * (size_t)p + k] = edge_index[4 * (size_t)i + k];
            }
        }
    }
}

// ---- exclusive scan of u32 (three launches: tile sums, scan of the sums by one workgroup, apply) --------------------------
#define GS2M_SCAN_TILE 4096u   // items per workgroup of 1024 threads (4 each)
GS2M_DEVICE unsigned mesh_wg_exclusive_scan_1024(unsigned v, unsigned* wave_sum /* LDS [16] */, unsigned* total) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = gs2m_shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // wave_sum may still be read by the previous use
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned base = 0, all = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < wave) base += wave_sum[k];
        all += wave_sum[k];
    }
    if (total) *total = all;
    return base + inc - v;
}
GS2M_KERNEL void __launch_bounds__(1024)
k_scan_tile_sums(const unsigned* __restrict__ in, unsigned n, unsigned* __restrict__ sums) {
    __shared__ unsigned wave_sum[16];
    const unsigned base = blockIdx.x * GS2M_SCAN_TILE + threadIdx.x * 4u;
    unsigned s = 0;
    for (unsigned k = 0; k < 4u; ++k) s += base + k < n ? in[base + k] : 0u;
    unsigned total = 0;
    (void)mesh_wg_exclusive_scan_1024(s, wave_sum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: exclusive scan of sums[m] in place; the grand total -> total_out[0]
GS2M_KERNEL void __launch_bounds__(1024)
k_scan_sums(unsigned* __restrict__ sums, unsigned m, unsigned* __restrict__ total_out) {
    __shared__ unsigned wave_sum[16];
    __shared__ unsigned carry;
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    for (unsigned b0 = 0; b0 < m; b0 += 1024u) {
        const unsigned i = b0 + threadIdx.x;
        const unsigned v = i < m ? sums[i] : 0u;
        unsigned total = 0;
        const unsigned ex = mesh_wg_exclusive_scan_1024(v, wave_sum, &total);
        const unsigned c = carry;
        if (i < m) sums[i] = c + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) total_out[0] = carry;
}
GS2M_KERNEL void __launch_bounds__(1024)
k_scan_apply(const unsigned* __restrict__ in, unsigned n, const unsigned* __restrict__ sums, unsigned* __restrict__ out) {
    __shared__ unsigned wave_sum[16];
    const unsigned base = blockIdx.x * GS2M_SCAN_TILE + threadIdx.x * 4u;
    unsigned v[4], s = 0;
    for (unsigned k = 0; k < 4u; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        s += v[k];
    }
    unsigned run = sums[blockIdx.x] + mesh_wg_exclusive_scan_1024(s, wave_sum, nullptr);
    for (unsigned k = 0; k < 4u; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// ---- connected components over shared edges ------------------------------------------------------------------------------
GS2M_DEVICE unsigned mesh_uf_find(unsigned* __restrict__ parent, unsigned i) {
    unsigned p = gs2m_load_agent(&parent[i]);
    while (p != i) {
        const unsigned g = gs2m_load_agent(&parent[p]);
        if (g != p) parent[i] = g;     // path halving (a benign race: any ancestor is a valid parent)
        i = p;
        p = g;
    }
    return i;
}
GS2M_DEVICE void mesh_uf_union(unsigned* __restrict__ parent, unsigned a, unsigned b) {
    for (;;) {
        a = mesh_uf_find(parent, a);
        b = mesh_uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        // hook the larger root under the smaller: the root of a component ends up its smallest triangle
        if (atomicCAS(&parent[b], b, a) == b) return;
    }
}
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_uf_init(unsigned n, unsigned* __restrict__ parent) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) parent[i] = i;
}
// every triangle registers its three undirected edges; hval[cell] = a triangle that carries the edge (the first to arrive),
// everybody else is united with it
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_uf_edges(const int* __restrict__ tri, unsigned n_tri, unsigned long long* __restrict__ hkeys, unsigned* __restrict__ hval,
                unsigned cap, unsigned* __restrict__ parent) {
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < n_tri; t += gridDim.x * 256u) {
        const unsigned v[3] = {(unsigned)tri[3 * (size_t)t], (unsigned)tri[3 * (size_t)t + 1], (unsigned)tri[3 * (size_t)t + 2]};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const unsigned a = v[e], b = v[(e + 1) % 3];
            const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
            const unsigned c = mesh_table_cell(hkeys, cap, ((unsigned long long)lo << 32) | hi);
            const unsigned prev = atomicCAS(&hval[c], 0xffffffffu, t);
            if (prev != 0xffffffffu && prev != t) mesh_uf_union(parent, prev, t);
        }
    }
}
// root of every triangle (the component's smallest triangle) + flag[t] = 1 where t is a root
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_uf_roots(unsigned n_tri, unsigned* __restrict__ parent, unsigned* __restrict__ root, unsigned* __restrict__ flag) {
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < n_tri; t += gridDim.x * 256u) {
        const unsigned r = mesh_uf_find(parent, t);
        root[t] = r;
        flag[t] = r == t ? 1u : 0u;
    }
}
// labels = rank of the root among the roots (pos = exclusive scan of flag); cluster sizes by atomics, aggregated per wave: the
// triangles of a wave mostly belong to ONE component (a scene is one big surface + debris), and 0.87 M single atomics on the
// big component's counter took 10 ms
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_uf_labels(unsigned n_tri, const unsigned* __restrict__ root, const unsigned* __restrict__ pos, int* __restrict__ labels,
                 unsigned long long* __restrict__ cluster_n) {
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned stride = gridDim.x * 256u;
    const unsigned rounds = (n_tri + stride - 1u) / stride;      // the same for every lane: the ballots below are collectives
    for (unsigned r = 0; r < rounds; ++r) {
        const unsigned t = r * stride + blockIdx.x * 256u + threadIdx.x;
        const bool have = t < n_tri;
        const unsigned l = have ? pos[root[t]] : 0xffffffffu;
        if (have) labels[t] = (int)l;
        unsigned long long todo = gs2m_ballot(have ? 1 : 0);
        while (todo != 0ull) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned ll = gs2m_shfl(l, leader);
            const unsigned long long same = gs2m_ballot(have && l == ll ? 1 : 0);
            if (lane == leader) atomicAdd(&cluster_n[ll], (unsigned long long)gs2m_popc64(same));
            todo &= ~same;
        }
    }
}

// ---- vertex normals (TriangleMesh.compute_vertex_normals, tsdf_utils.py:110) ----------------------------------------------------
// Bit-identical to the numpy statement in gs2mesh_amd/mesh.py (this header is compiled with -ffp-contract=off):
//   triangle t:  n = np.cross(v1 - v0, v2 - v0);  n / (|n| > 0 ? |n| : 1),  |n| = sqrt((x*x + y*y) + z*z)  (np.linalg.norm)
//   vertex v:    the sum, from 0.0, of the normals of its incidences in np.add.at order -- every (t, k = 0) with tri[t][0] == v in
//                ascending t, then k = 1, then k = 2 -- normalised the same way.
// The order is the incidence number i = k * n_tri + t.  The incidences are bucketed by vertex with atomics (arbitrary order inside
// a bucket), then every bucket is sorted by i with merge passes of doubling width (runs never cross a bucket; ceil(log2(max
// degree)) passes: any degree), and one thread per vertex sums its bucket in that order.
GS2M_DEVICE double mesh_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
GS2M_DEVICE bool mesh_tri_ok(const int* __restrict__ tri, size_t t, unsigned nv) {
    return (unsigned)tri[3 * t] < nv && (unsigned)tri[3 * t + 1] < nv && (unsigned)tri[3 * t + 2] < nv;
}
// triangle normals + vertex degrees; bad[0] = 1 when a triangle names a vertex outside [0, nv) (the triangle is skipped)
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_tri_normals(const double* __restrict__ v, unsigned nv, const int* __restrict__ tri, unsigned nt, double* __restrict__ tn,
                   unsigned* __restrict__ deg, unsigned* __restrict__ bad) {
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < nt; t += gridDim.x * 256u) {
        if (!mesh_tri_ok(tri, t, nv)) {
            atomicOr(bad, 1u);
            continue;
        }
        const size_t i0 = (size_t)tri[3 * (size_t)t], i1 = (size_t)tri[3 * (size_t)t + 1], i2 = (size_t)tri[3 * (size_t)t + 2];
        const double a0 = v[3 * i1] - v[3 * i0], a1 = v[3 * i1 + 1] - v[3 * i0 + 1], a2 = v[3 * i1 + 2] - v[3 * i0 + 2];
        const double b0 = v[3 * i2] - v[3 * i0], b1 = v[3 * i2 + 1] - v[3 * i0 + 1], b2 = v[3 * i2 + 2] - v[3 * i0 + 2];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        const double ln = mesh_norm3(c0, c1, c2);
        const double d = ln > 0.0 ? ln : 1.0;
        tn[3 * (size_t)t] = c0 / d;
        tn[3 * (size_t)t + 1] = c1 / d;
        tn[3 * (size_t)t + 2] = c2 / d;
        atomicAdd(&deg[i0], 1u);
        atomicAdd(&deg[i1], 1u);
        atomicAdd(&deg[i2], 1u);
    }
}
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_deg_max(const unsigned* __restrict__ deg, unsigned nv, unsigned* __restrict__ max_deg) {
    unsigned m = 0u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nv; i += gridDim.x * 256u) m = deg[i] > m ? deg[i] : m;
    if (m) atomicMax(max_deg, m);
}
// incidence i = k * nt + t into the bucket of its vertex (off = exclusive scan of deg; fill starts at 0); owner[slot] = vertex
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_incidence_scatter(const int* __restrict__ tri, unsigned nv, unsigned nt, const unsigned* __restrict__ off, unsigned* __restrict__ fill,
                         unsigned* __restrict__ list, unsigned* __restrict__ owner) {
    const unsigned n = 3u * nt;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned k = i / nt, t = i - k * nt;
        if (!mesh_tri_ok(tri, t, nv)) continue;
        const unsigned vtx = (unsigned)tri[3 * (size_t)t + k];
        const unsigned slot = off[vtx] + atomicAdd(&fill[vtx], 1u);
        list[slot] = i;
        owner[slot] = vtx;
    }
}
// one merge pass: inside every bucket, runs of `width` sorted entries are merged pairwise (src -> dst).  Entry x of run r lands
// at its index in the run + the number of entries of the partner run below it (the entries of a bucket are distinct).
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_bucket_merge(unsigned n, unsigned width, const unsigned* __restrict__ off, const unsigned* __restrict__ deg,
                    const unsigned* __restrict__ owner, const unsigned* __restrict__ src, unsigned* __restrict__ dst) {
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const unsigned vtx = owner[p], s = off[vtx], len = deg[vtx];
        const unsigned q = p - s, r = q / width, x = src[p];
        const unsigned long long pair = (unsigned long long)(r & ~1u) * width;
        unsigned long long lo = (r & 1u) ? pair : pair + width;
        unsigned long long hi = (r & 1u) ? pair + width : pair + 2ull * width;
        hi = hi < len ? hi : len;
        lo = lo < hi ? lo : hi;
        unsigned below = 0u;     // lower bound of x in the partner run [lo, hi)
        unsigned long long a = lo, b = hi;
        while (a < b) {
            const unsigned long long m = (a + b) >> 1;
            if (src[s + m] < x) a = m + 1;
            else b = m;
        }
        below = (unsigned)(a - lo);
        dst[s + (unsigned)pair + (q - r * width) + below] = x;
    }
}
// per vertex: the sum of its incidences' triangle normals in bucket (= np.add.at) order, normalised.  One thread walks the whole
// bucket: the additions are a serial chain by definition (floating-point addition does not associate, and the result must be the
// one np.add.at's left-to-right sum rounds to), so a vertex of degree d costs d dependent adds -- a tree or segmented reduction
// would round differently.  The loads of the chain do not depend on the sum and run ahead of it.  Marching-cubes meshes have
// degrees of about 6; a mesh with one vertex of very high degree makes this launch as long as that vertex's chain.
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_vertex_sum(unsigned nv, unsigned nt, const unsigned* __restrict__ off, const unsigned* __restrict__ deg,
                  const unsigned* __restrict__ list, const double* __restrict__ tn, double* __restrict__ vn) {
    for (unsigned vtx = blockIdx.x * 256u + threadIdx.x; vtx < nv; vtx += gridDim.x * 256u) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        const unsigned b = off[vtx], e = b + deg[vtx];
        for (unsigned j = b; j < e; ++j) {
            const unsigned i = list[j];
            const size_t t = i - (i / nt) * nt;
            s0 += tn[3 * t];
            s1 += tn[3 * t + 1];
            s2 += tn[3 * t + 2];
        }
        const double ln = mesh_norm3(s0, s1, s2);
        const double d = ln > 0.0 ? ln : 1.0;
        vn[3 * (size_t)vtx] = s0 / d;
        vn[3 * (size_t)vtx + 1] = s1 / d;
        vn[3 * (size_t)vtx + 2] = s2 / d;
    }
}
