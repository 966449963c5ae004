// VSL_DEBUG_TIMING phase stamps: thread 0 of workgroup (0, 0) of an instrumented kernel writes the shader clock at its phase boundaries, and the
// launcher prints the differences.  Compiled in only with -DVSL_STAMPS (vslnet_amd.build.build(stamps=True) -> libvslnet_hip_stamps.so; run with
// VSLNET_HIP_LIB=<that file> VSL_DEBUG_TIMING=1): the product library carries none of it -- even a disabled stamp reads its enable flag from
// memory and waits for it (vmcnt(0)), which drains every prefetch in flight at that point.
// Each kernel unit that includes this header has its own buffer and flag: a static device variable is per translation unit, and the library is
// not built with relocatable device code.  (The harness stamps of kernels_split.hip / kernels_wgrad.hip are another facility: per wave, read by
// tools/ubench.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

namespace vsl {
namespace stamps {

#ifdef VSL_STAMPS
constexpr int NSTAMPS = 40;
static __device__ long long g_buf[NSTAMPS];
static __device__ int g_on = 0;
#define STAMP(k) do { if (vsl::stamps::g_on && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) vsl::stamps::g_buf[k] = clock64(); } while (0)
// reads VSL_DEBUG_TIMING once and switches this unit's stamps on
static inline bool enabled() {
    static const bool on = [] {
        const bool v = getenv("VSL_DEBUG_TIMING") != nullptr;
        if (v) { const int one = 1; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_on), &one, sizeof one); }
        return v;
    }();
    return on;
}
// "[name cycles] d(i0 + 1) .. d(i1 - 1) | total": the intervals between stamps i0 .. i1 - 1 of the last launch on `s`; at most `left` times
static inline void report_range(const char* name, int i0, int i1, hipStream_t s, int& left) {
    if (left <= 0) return;
    long long h[NSTAMPS];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_buf), sizeof h);
    fprintf(stderr, "[%s cycles]", name);
    for (int i = i0 + 1; i < i1; ++i) fprintf(stderr, " %lld", h[i] - h[i - 1]);
    fprintf(stderr, " | total %lld\n", h[i1 - 1] - h[i0]);
    --left;
}
#else
#define STAMP(k) do { } while (0)
static inline bool enabled() { return false; }
static inline void report_range(const char*, int, int, hipStream_t, int&) {}
#endif
static inline void report(const char* name, int nst, hipStream_t s, int& left) { report_range(name, 0, nst, s, left); }      // stamps 0 .. nst - 1

}  // namespace stamps
}  // namespace vsl
