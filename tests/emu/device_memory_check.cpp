// device_memory_check.cpp -- stand-alone check of gs2mesh_amd/csrc/device_memory.h on the emulator's host API.
// TEST INFRASTRUCTURE ONLY (built and run by tests/test_device_memory.py).  Exit status 0 and "ok" = every case passed.
#include <stdarg.h>

#include <string>

#include "platform.h"

#include "device_memory.h"

static std::string g_err;
void gs2m_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

static unsigned pow2_at_least(unsigned long long n) {   // as in tsdf_api.hip
    unsigned c = 1024u;
    while ((unsigned long long)c < n && c < 0x80000000u) c <<= 1;
    return c;
}

struct Span {
    const char* p;
    size_t bytes;
};
// every sub-buffer 256-byte aligned, inside the arena, in order and apart from the one before it
static void check_spans(const ScratchArena& A, const Span* s, int n) {
    const char* end = A.base() + A.capacity();
    CHECK(A.base() != nullptr);
    for (int i = 0; i < n; ++i) {
        CHECK(((uintptr_t)s[i].p & 255u) == 0);
        CHECK(s[i].p >= A.base() && s[i].p + s[i].bytes <= end);
        if (i) CHECK(s[i - 1].p + s[i - 1].bytes <= s[i].p);
    }
}
#define SPAN(ptr, count) Span{reinterpret_cast<const char*>(ptr), sizeof(*(ptr)) * (size_t)(count)}

// the four layouts, as their call sites declare them
static void extraction_layout(ScratchArena& A, unsigned n) {   // gs2m_tsdf_extract_mesh, n = 3 * triangles
    const unsigned cap = pow2_at_least(2ull * n), m = (n + 4095u) / 4096u;
    double *soup_v, *soup_c;
    int *soup_e, *small;
    unsigned long long* hkeys;
    unsigned *hfirst, *cell_of, *flag, *pos, *scratch;
    const int rc = A.carve(arena_sub(soup_v, 3 * (size_t)n), arena_sub(soup_c, 3 * (size_t)n), arena_sub(soup_e, 4 * (size_t)n),
                           arena_sub(hkeys, cap), arena_sub(hfirst, cap), arena_sub(cell_of, n), arena_sub(flag, n), arena_sub(pos, n),
                           arena_sub(scratch, (size_t)m + 2), arena_sub(small, 4));
    CHECK(rc == 0);
    if (rc) return;
    const Span s[] = {SPAN(soup_v, 3 * (size_t)n), SPAN(soup_c, 3 * (size_t)n), SPAN(soup_e, 4 * (size_t)n), SPAN(hkeys, cap),
                      SPAN(hfirst, cap), SPAN(cell_of, n), SPAN(flag, n), SPAN(pos, n), SPAN(scratch, m + 2), SPAN(small, 4)};
    check_spans(A, s, 10);
}
static void cluster_layout(ScratchArena& A, unsigned nt) {   // gs2m_mesh_cluster
    const unsigned cap = pow2_at_least(6ull * nt), m = (nt + 4095u) / 4096u;
    unsigned long long* hkeys;
    unsigned *hval, *parent, *root, *flag, *pos, *scratch;
    const int rc = A.carve(arena_sub(hkeys, cap), arena_sub(hval, cap), arena_sub(parent, nt), arena_sub(root, nt), arena_sub(flag, nt),
                           arena_sub(pos, nt), arena_sub(scratch, (size_t)m + 2));
    CHECK(rc == 0);
    if (rc) return;
    const Span s[] = {SPAN(hkeys, cap), SPAN(hval, cap), SPAN(parent, nt), SPAN(root, nt), SPAN(flag, nt), SPAN(pos, nt), SPAN(scratch, m + 2)};
    check_spans(A, s, 7);
}
static void normals_layout(ScratchArena& A, unsigned nv, unsigned ni) {   // gs2m_mesh_vertex_normals
    const unsigned m = (nv + 4095u) / 4096u;
    unsigned *deg, *off, *fill, *list, *list2, *owner, *scratch, *small;
    const int rc = A.carve(arena_sub(deg, nv), arena_sub(off, nv), arena_sub(fill, nv), arena_sub(list, ni), arena_sub(list2, ni),
                           arena_sub(owner, ni), arena_sub(scratch, (size_t)m + 2), arena_sub(small, 2));
    CHECK(rc == 0);
    if (rc) return;
    const Span s[] = {SPAN(deg, nv), SPAN(off, nv), SPAN(fill, nv), SPAN(list, ni), SPAN(list2, ni), SPAN(owner, ni), SPAN(scratch, m + 2), SPAN(small, 2)};
    check_spans(A, s, 8);
}
static void png_layout(ScratchArena& A, size_t n, size_t nseg, size_t max_chunks) {   // gs2m_png_encode
    struct Seg { unsigned u[4]; unsigned long long s0, s1; };   // sizes of PngSeg / PngImg (png_encode.hip)
    struct Img { unsigned long long idat_len, total; };
    const size_t nsegs = n * nseg;
    Seg* segs;
    unsigned *codes, *hdr, *chunk_crc;
    unsigned long long* seg_off;
    Img* imgs;
    const int rc = A.carve(arena_sub(segs, nsegs), arena_sub(codes, nsegs * 260), arena_sub(hdr, nsegs * 128), arena_sub(seg_off, nsegs),
                           arena_sub(imgs, n), arena_sub(chunk_crc, n * max_chunks));
    CHECK(rc == 0);
    if (rc) return;
    const Span s[] = {SPAN(segs, nsegs), SPAN(codes, nsegs * 260), SPAN(hdr, nsegs * 128), SPAN(seg_off, nsegs), SPAN(imgs, n), SPAN(chunk_crc, n * max_chunks)};
    check_spans(A, s, 6);
}

int main() {
    {   // grow-only: no reallocation and a stable pointer while need <= capacity
        DeviceBuffer<float> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(1000) == 0);
        CHECK(b.get() != nullptr && b.capacity() == 1000 + 125 + 64);   // the headroom the backward's arena_bytes reports
        float* p = b.get();
        const size_t cap = b.capacity();
        CHECK(b.reserve(10) == 0 && b.get() == p && b.capacity() == cap);
        CHECK(b.reserve(cap) == 0 && b.get() == p && b.capacity() == cap);
        CHECK(b.reserve(cap + 1) == 0 && b.capacity() == cap + 1 + (cap + 1) / 8 + 64);
        CHECK(b.reserve(0) == 0 && b.capacity() == cap + 1 + (cap + 1) / 8 + 64);
        DeviceBuffer<float> e;
        CHECK(e.reserve(0) == 0 && e.get() != nullptr && e.capacity() == 64);   // an empty request still yields a pointer
        DeviceBuffer<double> x;
        CHECK(x.reserve_exact(7) == 0 && x.capacity() == 7);
        double* q = x.get();
        CHECK(x.reserve_exact(7) == 0 && x.get() == q);
    }
    {   // a request that cannot be met: 1, error set, buffer empty; a small one then works.  Both from empty and from filled.
        DeviceBuffer<char> b;
        g_err.clear();
        CHECK(b.reserve(SIZE_MAX / 16) == 1);
        CHECK(!g_err.empty() && b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(100) == 0 && b.get() != nullptr && b.capacity() >= 100);
        CHECK(b.reserve(SIZE_MAX / 16) == 1 && b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(50) == 0 && b.capacity() >= 50);
        DeviceBuffer<double> d;   // the byte count does not fit a size_t
        CHECK(d.reserve(SIZE_MAX / 16) == 1 && d.get() == nullptr && d.capacity() == 0);
        CHECK(d.reserve_exact(SIZE_MAX / 4) == 1 && d.get() == nullptr);
        CHECK(d.reserve(SIZE_MAX - 3) == 1 && d.get() == nullptr);   // need + need / 8 wraps
        CHECK(d.reserve(3) == 0 && d.get() != nullptr);
        PinnedBuffer<unsigned> h;
        CHECK(h.reserve(SIZE_MAX / 2) == 1 && h.get() == nullptr && h.capacity() == 0);
        CHECK(h.reserve(4) == 0 && h.get() != nullptr && h.capacity() == 4);
        h.get()[3] = 7u;
        unsigned* hp = h.get();
        CHECK(h.reserve(2) == 0 && h.get() == hp && hp[3] == 7u);
    }
    {   // the arena: the four real layouts at their smallest sizes, then reuse after a larger and a smaller request
        ScratchArena A;
        CHECK(A.base() == nullptr && A.capacity() == 0);
        extraction_layout(A, 3);
        extraction_layout(A, 4097);
        const char* base = A.base();
        const size_t cap = A.capacity();
        CHECK(cap > 0 && base != nullptr);
        extraction_layout(A, 3);
        CHECK(A.base() == base && A.capacity() == cap);   // larger, then smaller: the allocation stays
        cluster_layout(A, 1);
        normals_layout(A, 1, 3);
        png_layout(A, 1, 1, 1);
        CHECK(A.base() == base && A.capacity() == cap);
        ScratchArena B;   // each layout on an arena of its own: the first request sizes it
        cluster_layout(B, 1);
        ScratchArena C;
        normals_layout(C, 1, 3);
        ScratchArena D;
        png_layout(D, 1, 1, 1);
        unsigned* big;
        g_err.clear();
        CHECK(D.carve(arena_sub(big, SIZE_MAX / 64)) == 1 && !g_err.empty() && D.capacity() == 0);
        png_layout(D, 1, 1, 1);
    }
    {   // events are recycled, and a drain adds the weights
        EventPool pool;
        hipEvent_t a = pool.get(), b = pool.get(), c = pool.get(), d = pool.get();
        CHECK(a && b && c && d && a != b && c != d);
        hipStream_t st = nullptr;
        (void)hipEventRecord(a, st);
        (void)hipEventRecord(b, st);
        (void)hipEventRecord(c, st);
        (void)hipEventRecord(d, st);
        pool.push(0, a, b);
        pool.push(1, c, d, 5);
        double ms[2] = {0.0, 0.0};
        int64_t launches[2] = {0, 0};
        pool.drain(ms, launches, 2);
        CHECK(launches[0] == 1 && launches[1] == 5 && ms[0] >= 0.0 && ms[1] >= 0.0);
        pool.drain(ms, launches, 2);   // nothing is counted twice
        CHECK(launches[0] == 1 && launches[1] == 5);
        hipEvent_t r[4] = {pool.get(), pool.get(), pool.get(), pool.get()};
        for (hipEvent_t e : r) CHECK(e == a || e == b || e == c || e == d);
        CHECK(r[0] != r[1] && r[0] != r[2] && r[0] != r[3] && r[1] != r[2] && r[1] != r[3] && r[2] != r[3]);
        hipEvent_t f = pool.get();   // the pool is empty again: a new event
        CHECK(f && f != a && f != b && f != c && f != d);
        (void)hipEventRecord(r[0], st);
        (void)hipEventRecord(r[1], st);
        pool.push(7, r[0], r[1], 3);   // a stage outside the table is dropped, its events still recycled
        pool.drain(ms, launches, 2);
        CHECK(launches[0] == 1 && launches[1] == 5);
        (void)hipEventRecord(r[2], st);
        (void)hipEventRecord(r[3], st);
        pool.push(0, r[2], r[3], 2);   // left live: the destructor destroys live and free events alike
        (void)hipEventDestroy(f);      // never pushed: not the pool's
    }
    {   // the stage timer: a pair per timed stage, counted with its weight; nothing recorded when timing is off
        EventPool pool;
        hipStream_t st = nullptr;
        { StageTimer tm(pool, true, st, 0, "check:touch", 3); }
        { StageTimer tm(pool, true, st, 1, "check:integrate", 3); }
        { StageTimer tm(pool, true, st, 1, "check:integrate"); }
        { StageTimer tm(pool, false, st, 0, "check:off", 7); }
        double ms[2] = {0.0, 0.0};
        int64_t launches[2] = {0, 0};
        pool.drain(ms, launches, 2);
        CHECK(launches[0] == 3 && launches[1] == 4 && ms[0] >= 0.0 && ms[1] >= 0.0);
    }
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
