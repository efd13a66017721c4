// api_check.h -- the error plumbing of the API files.  Host code only.
//
//   gs2m_set_error        its one declaration (defined in raster_api.hip; the stand-alone host programs of the tests define their own)
//   GS2M_HIPCHK           a HIP call that sets the error and returns 1 when it fails
//   gs2m_scratch_refused  the contract of an entry point that works in the caller's scratch
#pragma once
#include <stdint.h>

#include "platform.h"

void gs2m_set_error(const char* fmt, ...);

#define GS2M_HIPCHK(expr)                                                                     \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            gs2m_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// The scratch of `fn` must be there, hold the `need` bytes that `sizer` returned and be aligned to `align` bytes (a power of two;
// 1 = the caller checks the alignment itself).  A NULL scratch is reported as 0 bytes.  1 = refused (the message is set).
inline int gs2m_scratch_refused(const char* fn, const char* sizer, const void* scratch, int64_t scratch_bytes, int64_t need,
                                unsigned align) {
    if (!scratch || scratch_bytes < need) {
        gs2m_set_error("%s: scratch of %lld bytes, %s asks for %lld", fn, (long long)(scratch ? scratch_bytes : 0), sizer,
                       (long long)need);
        return 1;
    }
    if ((uintptr_t)scratch & (uintptr_t)(align - 1u)) {
        gs2m_set_error("%s: scratch must be %u-byte aligned", fn, align);
        return 1;
    }
    return 0;
}
