// Coarse-to-fine corpus search, the coarse half (gfx950): one relevance score per (query, video) pair from the highlight score, and the M best videos of
// every query (include/vslnet_hip.h, vsl_highlight_pairs / vsl_select_topm).  Neither kernel has an atomic on a float or on global memory; both are pure
// functions of their inputs: the same bits on every run and for every position of a pair / a group in the call.
#include "common.hpp"
#include "launch.hpp"
#include "rank_reduce.hpp"

namespace vsl {

// ---- k_pair_relevance: (B, T) highlight scores -> one float per pair.  One wave per pair, four pairs per workgroup; the reduction and the order of its
// additions: rank_reduce.hpp pair_row_reduce (shared with the training loss, kernels_group_loss.hip).
__global__ __launch_bounds__(256) void k_pair_relevance(RelevanceArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;                                       // (wave-uniform; no barrier in this kernel)
    const float* h = a.hscore + (size_t)b * a.T;
    const float* m = a.vmask + (size_t)b * a.T;
    float best, sum;
    int cnt;
    pair_row_reduce(h, m, a.T, lane, best, sum, cnt);
    if (lane != 0) return;
    const float r = pair_row_relevance(best, sum, cnt, a.mean);
    const size_t o = a.ld > 0 ? (size_t)a.qidx[b] * (size_t)a.ld + (size_t)a.vidx[b] : (size_t)b;
    a.out[o] = r;
}

void launch_pair_relevance(const RelevanceArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_pair_relevance, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
}

// ---- k_select_topm: the first min(M, N) indices of every row in the order (key descending, index ascending), ranked.
// a float as an unsigned integer of the same order (larger key <-> larger integer); -0.0 has been folded into +0.0 by `key + 0.0f`
__device__ __forceinline__ uint32_t topm_ordered(float key) {
    const uint32_t u = __float_as_uint(key + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float topm_key(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// inclusive prefix sum of v over the 256 threads (thread order), `total` = the sum over all of them.  wsum: 4 ints of LDS, free again on return.
__device__ __forceinline__ int topm_scan(int v, int* wsum, int tid, int& total) {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    const int s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
    __syncthreads();
    total = s0 + s1 + s2 + s3;
    return v + (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
}

// One 256-thread workgroup per group (row).
//   1. four 8-bit histogram passes over the row's ordered integers, most significant digit first (integer LDS adds: a count does not depend on the order
//      of its increments), find the threshold tau = the take-th largest integer and `ties` = how many elements equal to tau are still to be taken;
//   2. one ordered pass, a block prefix scan per 256 elements: every element above tau, and the first `ties` elements equal to tau in ascending index,
//      go into an LDS array as (ordered key << 32 | ~index);
//   3. a bitonic sort of those <= 1024 words, descending: key descending, then index ascending -- a strict total order, so the slot an element took in
//      step 2 cannot show in the output.
// Every loop is bounded by N and TOPM_MAX_M.  NaN keys are ordered by their bits (unspecified but terminating).
__global__ __launch_bounds__(256) void k_select_topm(SelectArgs a) {
    __shared__ unsigned long long cand[TOPM_MAX_M];
    __shared__ int hist[256];
    __shared__ int wsum[4];
    __shared__ int sel[2];
    const int g = blockIdx.x, tid = threadIdx.x, N = a.N;
    const float* row = a.key + (size_t)g * a.ld;
    const int take = min(a.M, N);                               // 1 <= take <= TOPM_MAX_M
    uint32_t prefix = 0, mask = 0;
    int k = take;                                               // tau is the k-th largest among the elements that match `prefix` under `mask`
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < N; i += 256) {
            const uint32_t u = topm_ordered(row[i]);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
        }
        __syncthreads();
        const int c = hist[255 - tid];                          // thread t owns digit 255 - t: the scan counts the elements with a digit at least its own
        int total;
        const int incl = topm_scan(c, wsum, tid, total);
        if (incl - c < k && k <= incl) { sel[0] = 255 - tid; sel[1] = k - (incl - c); }      // (exactly one thread: 1 <= k <= total)
        __syncthreads();
        prefix |= (uint32_t)sel[0] << shift;
        mask |= 255u << shift;
        k = sel[1];
        __syncthreads();                                        // (sel is read before the next pass may write it)
    }
    const uint32_t tau = prefix;
    const int ties = k, n_gt = take - ties;
    int n2 = 1;
    while (n2 < take) n2 <<= 1;                                 // the sort's size: the power of two at or above `take`, <= TOPM_MAX_M
    for (int i = take + tid; i < n2; i += 256) cand[i] = 0ull;  // padding: behind every real entry (a real entry's low word is ~index >= 2^31)
    int run_gt = 0, run_tie = 0;
    for (int base = 0; base < N && (run_gt < n_gt || run_tie < ties); base += 256) {         // (block-uniform condition)
        const int i = base + tid;
        uint32_t u = 0;
        int gt = 0, tie = 0;
        if (i < N) { u = topm_ordered(row[i]); gt = u > tau; tie = u == tau; }
        int total;
        const int incl = topm_scan(gt | (tie << 16), wsum, tid, total);       // both counts in one scan (each at most 256)
        const int gt_before = run_gt + ((incl & 0xffff) - gt), tie_before = run_tie + ((incl >> 16) - tie);
        const unsigned long long word = ((unsigned long long)u << 32) | (uint32_t)~(uint32_t)i;
        if (gt) cand[gt_before] = word;                         // (gt_before < n_gt: exactly n_gt elements lie above tau)
        else if (tie && tie_before < ties) cand[n_gt + tie_before] = word;
        run_gt += total & 0xffff;
        run_tie += total >> 16;
    }
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j >= 1; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += 256) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long x = cand[lo], y = cand[hi];
                const bool desc = (lo & kk) == 0;
                if (desc ? x < y : x > y) { cand[lo] = y; cand[hi] = x; }
            }
            __syncthreads();
        }
    for (int r = tid; r < a.M; r += 256) {
        const size_t o = (size_t)g * a.M + r;
        if (r < take) {
            const unsigned long long w = cand[r];
            a.out_index[o] = (int32_t)~(uint32_t)w;
            a.out_key[o] = topm_key((uint32_t)(w >> 32));
        } else {                                                // slots from count on: -1, 0
            a.out_index[o] = -1;
            a.out_key[o] = 0.f;
        }
    }
    if (tid == 0) a.out_count[g] = take;
}

void launch_select_topm(const SelectArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_select_topm, dim3(a.G), dim3(256), 0, s, a);
}

}  // namespace vsl
