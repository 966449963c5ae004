// Training through a shared video encoding (vsl_forward_shared / vsl_backward_shared): the grouping of B queries by their video and the reduction
// of the encoding's gradient from queries to videos.  gfx950 only.  No floating-point atomics: every sum runs in ascending query order.
#include "common.hpp"
#include "launch.hpp"

namespace vsl {

// CSR of the grouping, built on the device because the index may be a device tensor the host never reads: start[n] .. start[n + 1] delimit the
// queries of video n in `members`, ascending b within a video.  ONE workgroup: a thread owns the videos n = tid, tid + 256, ..; it counts its
// videos' queries, thread 0 turns the counts into offsets, and every thread lists its videos' queries in order of b.  B reads of the index per
// video and pass (the index stays in L1 / L2: B ints); the launch sits on the forward's pack stream, off the dependent chain.
// An index outside [0, N) matches no video: that query is in no group (its dC is never summed); the reads of C through such an index are the
// caller's precondition (vslnet_hip.h).
__global__ __launch_bounds__(256) void k_group_csr(const int* __restrict__ vidx, int B, int N, int* __restrict__ start, int* __restrict__ members) {
    const int tid = threadIdx.x;
    for (int n = tid; n < N; n += 256) {
        int cnt = 0;
        for (int b = 0; b < B; ++b) cnt += vidx[b] == n;
        start[n + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        start[0] = 0;
        for (int n = 0; n < N; ++n) { run += start[n + 1]; start[n + 1] = run; }
    }
    __syncthreads();
    for (int n = tid; n < N; n += 256) {
        int o = start[n];
        for (int b = 0; b < B; ++b)
            if (vidx[b] == n) members[o++] = b;
    }
}

void launch_group_csr(const int* vidx, int B, int N, int* start, int* members, hipStream_t s) {
    VSL_LAUNCH(k_group_csr, dim3(1), dim3(256), 0, s, vidx, B, N, start, members);
}

// dCv[n] = sum over the queries b of video n, ascending b, of dC[b]: (B, T, 128) -> (N, T, 128).  Memory bound: B T 128 floats read once, N T 128
// written.  One workgroup per (tile of GS_ROWS rows, video): a thread keeps GS_ROWS / 8 float4 accumulators and walks the group in member order,
// 16-byte loads and stores.  A video without a query gets zeros.
constexpr int GS_ROWS = 32, GS_Q = GS_ROWS * (D / 4) / 256;       // rows per workgroup ; float4 per thread
__global__ __launch_bounds__(256) void k_group_sum(const float* __restrict__ dC, const int* __restrict__ start, const int* __restrict__ members,
                                                   float* __restrict__ dCv, int T) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const size_t per = (size_t)T * (D / 4);                       // float4 per sample
    const size_t i0 = (size_t)blockIdx.x * (GS_ROWS * (D / 4)) + tid;
    const int m0 = start[n], m1 = start[n + 1];
    const float4* __restrict__ src = reinterpret_cast<const float4*>(dC);
    float4 acc[GS_Q];
#pragma unroll
    for (int q = 0; q < GS_Q; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int m = m0; m < m1; ++m) {
        const size_t base = (size_t)members[m] * per;
        float4 v[GS_Q];
#pragma unroll
        for (int q = 0; q < GS_Q; ++q) {
            const size_t i = i0 + (size_t)q * 256;
            v[q] = i < per ? src[base + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < GS_Q; ++q) { acc[q].x += v[q].x; acc[q].y += v[q].y; acc[q].z += v[q].z; acc[q].w += v[q].w; }
    }
    float4* __restrict__ dst = reinterpret_cast<float4*>(dCv) + (size_t)n * per;
#pragma unroll
    for (int q = 0; q < GS_Q; ++q) {
        const size_t i = i0 + (size_t)q * 256;
        if (i < per) dst[i] = acc[q];
    }
}

void launch_group_sum(const float* dC, const int* start, const int* members, float* dCv, int N, int T, hipStream_t s) {
    VSL_LAUNCH(k_group_sum, dim3((T + GS_ROWS - 1) / GS_ROWS, N), dim3(256), 0, s, dC, start, members, dCv, T);
}

}  // namespace vsl
