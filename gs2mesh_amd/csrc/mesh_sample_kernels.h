// mesh_sample_kernels.h -- gs2m_mesh_sample_count / _emit: the DTU evaluation's mesh -> point set step
// (evaluation/DTU/eval_code/eval.py:10-19, 54-71): all vertices, then for every triangle of non-zero area a regular
// barycentric grid whose pitch follows the density threshold.  The reference builds the grids with a multiprocessing pool.
//
// One lane per triangle, f64, every operation rounded on its own (this header is compiled into points_kernels.hip, built
// with -ffp-contract=off; sqrt and the division are IEEE).  include/gs2mesh_amd.h states the arithmetic; tests/
// mesh_sample_statement.py is its numpy form and is pinned, bit for bit, to points the reference's own function returned.
// The count pass and the emit pass run the same loop, so they agree on every triangle by construction.
#pragma once

#define MESH_SAMPLE_MAX_GRID 1048576.0     // (N1 + 1) * (N2 + 1) above this: the triangle is refused, not sampled

struct MeshSampleTri {
    double v0[3], a[3], b[3];
    double n1, n2;             // grid counts as the reference holds them: floats
    int i1, i2;                // the same as loop bounds; -1, -1 when the triangle gets no grid
    unsigned status;
};

GS2M_DEVICE MeshSampleTri mesh_sample_setup(unsigned nv, const double* __restrict__ verts, const int* __restrict__ tri, unsigned t,
                                            double density) {
    MeshSampleTri s;
    s.i1 = s.i2 = -1;
    s.n1 = s.n2 = 0.0;
    s.status = 0u;
    const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if ((unsigned)i0 >= nv || (unsigned)i1 >= nv || (unsigned)i2 >= nv) {
        s.status = GS2M_MESH_SAMPLE_INDEX;
        for (int k = 0; k < 3; ++k) s.v0[k] = s.a[k] = s.b[k] = 0.0;
        return s;
    }
    for (int k = 0; k < 3; ++k) {
        s.v0[k] = verts[3 * (size_t)i0 + k];
        s.a[k] = verts[3 * (size_t)i1 + k] - s.v0[k];
        s.b[k] = verts[3 * (size_t)i2 + k] - s.v0[k];
    }
    const double l1 = sqrt((s.a[0] * s.a[0] + s.a[1] * s.a[1]) + s.a[2] * s.a[2]);
    const double l2 = sqrt((s.b[0] * s.b[0] + s.b[1] * s.b[1]) + s.b[2] * s.b[2]);
    const double cx = s.a[1] * s.b[2] - s.a[2] * s.b[1];
    const double cy = s.a[2] * s.b[0] - s.a[0] * s.b[2];
    const double cz = s.a[0] * s.b[1] - s.a[1] * s.b[0];
    const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area2 > 0.0)) return s;
    const double thr = density * sqrt(l1 * l2 / area2);
    s.n1 = floor(l1 / thr);
    s.n2 = floor(l2 / thr);
    // a NaN or negative count (a NaN coordinate, a density that is not positive) gives an empty grid in the reference too
    if (!(s.n1 >= 0.0) || !(s.n2 >= 0.0)) return s;
    if (!((s.n1 + 1.0) * (s.n2 + 1.0) <= MESH_SAMPLE_MAX_GRID)) {
        s.status = GS2M_MESH_SAMPLE_CAP;
        return s;
    }
    s.i1 = (int)s.n1;
    s.i2 = (int)s.n2;
    return s;
}

// the grid walk shared by the two passes: emit(k, c0, c1) for the k-th kept node, i major, j minor; returns the count
template <typename Emit>
GS2M_DEVICE unsigned mesh_sample_walk(const MeshSampleTri& s, Emit emit) {
    unsigned k = 0;
    const double d1 = s.n1 > 1e-7 ? s.n1 : 1e-7, d2 = s.n2 > 1e-7 ? s.n2 : 1e-7;
    for (int i = 0; i <= s.i1; ++i) {
        const double c0 = ((double)i + 0.5) / d1;
        for (int j = 0; j <= s.i2; ++j) {
            const double c1 = ((double)j + 0.5) / d2;
            if (c0 + c1 < 1.0) emit(k++, c0, c1);
        }
    }
    return k;
}

// state[0] = total (u64), low word of state[1] = status bits; both zeroed by the caller on the stream
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_sample_count(unsigned nv, const double* __restrict__ verts, const int* __restrict__ tri, unsigned nt, double density,
                    unsigned* __restrict__ counts, unsigned long long* __restrict__ state) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nt) return;
    const MeshSampleTri s = mesh_sample_setup(nv, verts, tri, t, density);
    const unsigned n = mesh_sample_walk(s, [](unsigned, double, double) {});
    counts[t] = n;
    if (n) atomicAdd(state, (unsigned long long)n);
    if (s.status) atomicOr((unsigned*)(state + 1), s.status);
}

// points[nv + total][3]: rows [0, nv) are the vertices (copied by the caller), the samples of triangle t start at row
// nv + offsets[t].  A row at or past `total` is never written, whatever counts and offsets hold.
GS2M_KERNEL void __launch_bounds__(256)
k_mesh_sample_emit(unsigned nv, const double* __restrict__ verts, const int* __restrict__ tri, unsigned nt, double density,
                   const unsigned* __restrict__ counts, const unsigned* __restrict__ offsets, unsigned long long total,
                   double* __restrict__ points) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nt) return;
    const unsigned n = counts[t];
    const unsigned long long off = offsets[t];
    if (n == 0u || off + n > total) return;
    const MeshSampleTri s = mesh_sample_setup(nv, verts, tri, t, density);
    double* out = points + 3 * ((size_t)nv + (size_t)off);
    mesh_sample_walk(s, [&](unsigned k, double c0, double c1) {
        if (k >= n) return;
        for (int a = 0; a < 3; ++a) out[3 * (size_t)k + a] = (s.a[a] * c0 + s.b[a] * c1) + s.v0[a];
    });
}
