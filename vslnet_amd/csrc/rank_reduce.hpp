// The row reduction of the video relevance (include/vslnet_hip.h, vsl_highlight_pairs) as a device function: k_pair_relevance (kernels_rank.hip)
// scores a pair with it at search time and k_group_loss_a (kernels_group_loss.hip) the same pair at training time -- one definition, the same bits.
#pragma once
#include "common.hpp"

namespace vsl {

// One wave reduces one (T) row of highlight scores over its VALID clips (mask != 0).  Lane l visits clips l, l + 64, ... in ascending order (its
// partial), then a 6-step xor butterfly joins the 64 partials: fp32 addition commutes, so every lane of a step forms the same sum and the order of
// the additions is a function of T alone -- not of the row, not of the run.  max is exact in any order.  Every lane returns the three results.
__device__ __forceinline__ void pair_row_reduce(const float* __restrict__ h, const float* __restrict__ m, int T, int lane, float& best, float& sum, int& cnt) {
    best = -INFINITY; sum = 0.f; cnt = 0;
    for (int t = lane; t < T; t += 64) {
        if (m[t] == 0.f) continue;
        const float v = h[t];
        best = fmaxf(best, v);
        sum += v;
        ++cnt;
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        best = fmaxf(best, __shfl_xor(best, x));
        sum += __shfl_xor(sum, x);
        cnt += __shfl_xor(cnt, x);
    }
}
// ... and the relevance from them: -inf without a valid clip, else the mean (one fp32 division) or the maximum
__device__ __forceinline__ float pair_row_relevance(float best, float sum, int cnt, int mean) {
    return cnt == 0 ? -INFINITY : mean ? sum / (float)cnt : best;
}

}  // namespace vsl
