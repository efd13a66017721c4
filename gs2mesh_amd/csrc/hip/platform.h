// platform.h (product build) -- the only platform the shipped library is built for:
// HIP on gfx950 (MI355X, CDNA4, wave64).  Kernels include "platform.h" and use the small
// vocabulary below; tests/emu/platform.h provides the same vocabulary on CPU fibers so the
// kernel SOURCE can be executed in the GPU-less build container (test infrastructure only,
// never linked into libgs2mesh_amd.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS2M_KERNEL __global__
#define GS2M_WAVES_PER_SIMD(n) __attribute__((amdgpu_waves_per_eu(n, n)))   // occupancy of a kernel by construction (register budget = 512 / n)
#define GS2M_DEVICE __device__ __forceinline__
#define GS2M_PLATFORM_NAME "hip-gfx950"

// Dynamic LDS, 16-byte aligned (guide G17: keep the dynamic-LDS base 16-B aligned).
#define GS2M_DYN_LDS(type, name)                                              \
    extern __shared__ __attribute__((aligned(16))) unsigned char gs2m_dyn_lds_raw[]; \
    type* name = reinterpret_cast<type*>(gs2m_dyn_lds_raw)

#define GS2M_LAUNCH(kernel, grid, block, lds_bytes, stream, ...) \
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)(stream), __VA_ARGS__)

// wave64 vocabulary
GS2M_DEVICE unsigned long long gs2m_ballot(int pred) { return __ballot(pred); }
// ballot of a predicate that is already a lane mask (no 0/1 materialisation + v_cmp_ne as __ballot(int) costs), and its
// inverse: a wave-uniform 64-bit mask used as a per-lane predicate (no instruction: the mask IS the v_cndmask operand)
GS2M_DEVICE unsigned long long gs2m_ballot_b(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
GS2M_DEVICE bool gs2m_lanes(unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }
// "does any ACTIVE lane satisfy pred?" inside divergent code (ballot under the execution mask).  Only ever used to skip
// work no lane needs: taking the branch when the answer is no must be harmless (the CPU emulator always answers yes).
GS2M_DEVICE bool gs2m_any_active_lane(bool pred) { return __builtin_amdgcn_ballot_w64(pred) != 0ull; }
GS2M_DEVICE int gs2m_lane() { return (int)(threadIdx.x & 63u); }
GS2M_DEVICE int gs2m_popc64(unsigned long long m) { return __popcll(m); }
template <typename T>
GS2M_DEVICE T gs2m_shfl(T v, int src_lane) { return __shfl(v, src_lane, 64); }
template <typename T>
GS2M_DEVICE T gs2m_shfl_xor(T v, int mask) { return __shfl_xor(v, mask, 64); }
template <typename T>
GS2M_DEVICE T gs2m_shfl_up(T v, int d) { return __shfl_up(v, d, 64); }

// Orders LDS traffic of ONE wave (producer lanes -> consumer lanes of the same wave): DS ops of a wave
// execute in order, so only the compiler must be fenced.
GS2M_DEVICE void gs2m_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Loads that bypass the (non-coherent) per-CU L1: see the latest value another CU published with an
// atomic (guide: relaxed agent-scope load = global_load sc1).
GS2M_DEVICE unsigned gs2m_load_agent(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GS2M_DEVICE unsigned long long gs2m_load_agent(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 4 bytes at an arbitrary byte address (gfx9+ global loads need no alignment)
GS2M_DEVICE unsigned gs2m_load_u32_unaligned(const unsigned char* p) {
    typedef unsigned __attribute__((aligned(1))) u32_u;
    return *reinterpret_cast<const u32_u*>(p);
}
// value known to be identical in all lanes -> SGPR (lets the compiler branch on the scalar unit)
GS2M_DEVICE int gs2m_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
GS2M_DEVICE int gs2m_syncthreads_count(int pred) { return __syncthreads_count(pred); }

// fast exp for the blend kernel: v_exp_f32(x * log2e) (documented tolerance in DESIGN.md)
GS2M_DEVICE float gs2m_fast_exp(float x) { return __expf(x); }
GS2M_DEVICE float gs2m_fast_log(float x) { return __logf(x); }
GS2M_DEVICE float gs2m_fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }  // v_rcp_f32 (1 ulp)
GS2M_DEVICE float gs2m_fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32 (1 ulp)
GS2M_DEVICE float gs2m_fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32 (flushes denormal results)
GS2M_DEVICE float gs2m_fast_log2(float x) { return __log2f(x); }
// a + b rounded on its own: never contracted into an FMA with a neighbouring product (two code shapes that must round alike)
// (HIP's __fadd_rn is a plain `a + b`, which -ffp-contract=fast may fuse with a product feeding it: one v_add_f32, by hand)
GS2M_DEVICE float gs2m_add_rn(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// ---- one (instance, quadrant) of the compositing loop (raster_blend.h, loop forms 2 and 3), as ONE block of GCN.
// Per lane it is exactly this (raster_blend.h states these lines as C++ for a platform without GS2M_HAS_BLEND_QUADRANT: the CPU
// emulator of the tests runs them; GEN 0 = plain, 2 = alpha cap, 1 = alpha cap + the power > 0 test of the general path):
//     if (q >= thr) {                                  // candidate: thr is QMIN, or 1.0 once the pixel is finished
//         alpha = exp2(q);  [GEN: alpha = min(0.99, alpha)]  [GEN 1: alpha = q > lo ? 0 : alpha]
//         w = T * alpha;  T = fma(-T, alpha, T);
//         if (T < 1e-4) { T = T + w; thr = 1.0; w = 0; }          // saturated: contribution dropped, pixel finished
//         C0 = fma(cr, w, C0);  C1 = fma(cg, w, C1);  C2 = fma(cb, w, C2);
//     }
// with the vector instructions the compiler emitted for those lines, in its order, under the execution mask.  What the
// block fixes is the scalar side, which the compiler's lowering of the two `if`s cannot be talked out of:
//   * no candidate in the wave: one taken branch over the block (as before);
//   * candidates: s_and_saveexec and straight on -- no s_cbranch_execz behind a mask that the branch above has just
//     proven non-empty;
//   * the saturation fix-up sits out of line (subsection 1 of the kernel's own text section: behind its s_endpgm), so the
//     common case is ONE NOT-TAKEN branch where the compiler laid out a taken branch around the rare block (and a second
//     dead s_cbranch_execz inside it).
// The execution mask is saved and restored by the block itself: it assumes nothing about the mask it is entered with.
// Wait states (CDNA3 ISA 4.5): v_exp_f32 -> VALU use 1 (the s_nop, or the v_cmp in GEN 1); v_cmp -> v_cndmask through
// VCC 2 (v_min + s_nop in GEN 1).  The block ends on VALU writes of C0..C2 / a SALU write of EXEC: nothing the
// compiler's code behind it must wait for.
#define GS2M_HAS_BLEND_QUADRANT 1
#define GS2M_BQ_HEAD_                                                                                                   \
    "v_cmp_ge_f32 vcc, %[q], %[thr]\n\t"                                                                                \
    "s_cbranch_vccz .Lgs2m_bq_skip%=\n\t"                                                                               \
    "s_and_saveexec_b64 %[sv], vcc\n\t"                                                                                 \
    "v_exp_f32 %[al], %[q]\n\t"
#define GS2M_BQ_TAIL_                                                                                                   \
    "v_mul_f32 %[w], %[T], %[al]\n\t"                                                                                   \
    "v_fma_f32 %[T], -%[T], %[al], %[T]\n\t"                                                                            \
    "v_cmp_gt_f32 vcc, 0x38d1b717, %[T]\n\t" /* 1e-4f > T */                                                            \
    "s_cbranch_vccnz .Lgs2m_bq_sat%=\n"                                                                                 \
    ".Lgs2m_bq_acc%=:\n\t"                                                                                              \
    "v_fmac_f32 %[c0], %[cr], %[w]\n\t"                                                                                 \
    "v_fmac_f32 %[c1], %[cg], %[w]\n\t"                                                                                 \
    "v_fmac_f32 %[c2], %[cb], %[w]\n\t"                                                                                 \
    "s_or_b64 exec, exec, %[sv]\n"                                                                                      \
    ".Lgs2m_bq_skip%=:\n\t"                                                                                             \
    ".subsection 1\n"                                                                                                   \
    ".Lgs2m_bq_sat%=:\n\t"                                                                                              \
    "s_and_saveexec_b64 %[sv2], vcc\n\t"                                                                                \
    "v_add_f32 %[T], %[T], %[w]\n\t"                                                                                    \
    "v_mov_b32 %[thr], 1.0\n\t"                                                                                         \
    "v_mov_b32 %[w], 0\n\t"                                                                                             \
    "s_or_b64 exec, exec, %[sv2]\n\t"                                                                                   \
    "s_branch .Lgs2m_bq_acc%=\n\t"                                                                                      \
    ".subsection 0"
#define GS2M_BQ_OPERANDS_                                                                                               \
    [thr] "+v"(thr), [T] "+v"(T), [c0] "+v"(C0), [c1] "+v"(C1), [c2] "+v"(C2), [al] "=&v"(al), [w] "=&v"(w),            \
        [sv] "=&s"(sv), [sv2] "=&s"(sv2)                                                                                \
        : [q] "v"(q), [lo] "v"(lo), [cr] "v"(cr), [cg] "v"(cg), [cb] "v"(cb)                                            \
        : "vcc", "scc"
template <int GEN>
GS2M_DEVICE void gs2m_blend_quadrant(const float q, const float lo, const float cr, const float cg, const float cb, float& thr,
                                     float& T, float& C0, float& C1, float& C2) {
    static_assert(GEN >= 0 && GEN <= 2, "0 plain, 1 general path, 2 alpha cap");
    float al, w;
    unsigned long long sv, sv2;
    if (GEN == 0)
        asm volatile(GS2M_BQ_HEAD_ "s_nop 0\n\t" GS2M_BQ_TAIL_ : GS2M_BQ_OPERANDS_);
    else if (GEN == 2)
        asm volatile(GS2M_BQ_HEAD_ "s_nop 0\n\t"
                                   "v_min_f32 %[al], 0x3f7d70a4, %[al]\n\t" /* min(0.99f, alpha) */
                     GS2M_BQ_TAIL_ : GS2M_BQ_OPERANDS_);
    else
        asm volatile(GS2M_BQ_HEAD_ "v_cmp_ngt_f32 vcc, %[q], %[lo]\n\t"
                                   "v_min_f32 %[al], 0x3f7d70a4, %[al]\n\t"
                                   "s_nop 0\n\t"
                                   "v_cndmask_b32 %[al], 0, %[al], vcc\n\t" /* q > lo ? 0 : alpha */
                     GS2M_BQ_TAIL_ : GS2M_BQ_OPERANDS_);
}
#undef GS2M_BQ_HEAD_
#undef GS2M_BQ_TAIL_
#undef GS2M_BQ_OPERANDS_
// keep a loop-invariant float in its VGPR (stops the compiler re-materialising int->float converts in hot loops)
#define GS2M_KEEP_F32(x) asm volatile("" : "+v"(x))
// a wave-uniform int the compiler must treat as an opaque scalar register (stops re-association of mask tests)
#define GS2M_OPAQUE_SGPR(x) asm volatile("" : "+s"(x))
#define GS2M_OPAQUE_VGPR(x) asm volatile("" : "+v"(x))   // a per-lane value the compiler must re-read (stops hoisting of loads addressed by it)
// instruction-scheduling fence (nothing moves across it)
// keeps a rarely taken, wave-uniform branch a BRANCH (stops the compiler turning it into selects executed every time)
#define GS2M_NO_IF_CONVERT() asm volatile("" ::: "memory")
#define GS2M_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)

// ---- LDS-DMA gather: lane l's 16 bytes at `g` land at lds_base[l] without passing through a VGPR
// (global_load_lds_dwordx4; completion is tracked by vmcnt: gs2m_wait_dma before the LDS is read)
GS2M_DEVICE void gs2m_global_load_lds16(const void* g, void* lds_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}
// shader clock (s_memtime): phase stamps of the profile builds
// One asm statement: the value is complete when the statement ends (the scalar-memory return is asynchronous -- a
// destination the compiler believes free would be overwritten later), and it waits for the scalar / LDS counter only, never
// for vector memory (the builtin made the compiler drain the record DMA at every stamp: 7.5x slower kernel).
GS2M_DEVICE unsigned long long gs2m_clock() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t));
    return t;
}
GS2M_DEVICE void gs2m_wait_dma() { __builtin_amdgcn_s_waitcnt(0x0f70); }  // s_waitcnt vmcnt(0)
