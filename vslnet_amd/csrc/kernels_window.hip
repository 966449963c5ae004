// Sliding windows over a long video (gfx950): the gather between VisualProjection over the video's feature rows, run ONCE per clip, and the encoder
// application over the (N, T) windows (include/vslnet_hip.h, vsl_encode_windows).  Window n is rows window_row[n] .. window_row[n] + window_len[n] - 1
// of the projected (rows, 128) buffer; the rows behind its length are what VisualProjection makes of a zero feature row.  The replicated
// (N, T, video_feature_dim) block of overlapping windows never exists.
#include "common.hpp"
#include "launch.hpp"

namespace vsl {

// One thread per 16 bytes: 32 threads copy one (128-float) row, a 256-thread workgroup eight rows of the (N T, 128) output.
//   - live row (t < window_len[n] and 0 <= window_row[n] + t < rows): out[n][t] = proj[window_row[n] + t], a 16-byte load and store;
//   - pad row (everything else -- a bad table therefore reads nothing outside proj): out[n][t] = 0 + bias in fp32, which is what both projection
//     kernels store for a zero feature row (k_vproj_fwd3: (0 + 0) + b ; k_vproj_fwd_bf16: 0 * 1 + b);
//   - mask[n][t] = t < window_len[n].
// Every offset is formed in size_t.
__global__ __launch_bounds__(256) void k_window_gather(WindowGatherArgs a) {
    const size_t r = (size_t)blockIdx.x * 8 + (threadIdx.x >> 5), R = (size_t)a.N * (size_t)a.T;
    if (r >= R) return;
    const int n = (int)(r / (size_t)a.T), t = (int)(r % (size_t)a.T), c = (threadIdx.x & 31) * 4;
    const int len = a.window_len[n];
    const long long src = (long long)a.window_row[n] + t;
    float4 v;
    if (t < len && src >= 0 && src < (long long)a.rows) {
        v = *reinterpret_cast<const float4*>(a.proj + (size_t)src * D + c);
    } else {
        const float* b = a.bias + c;              // (the bias sits at a float offset of the parameter bucket: four 4-byte loads)
        v = make_float4(0.f + b[0], 0.f + b[1], 0.f + b[2], 0.f + b[3]);
    }
    *reinterpret_cast<float4*>(a.out + r * D + c) = v;
    if ((threadIdx.x & 31) == 0) a.mask[r] = t < len ? 1.f : 0.f;
}

void launch_window_gather(const WindowGatherArgs& a, hipStream_t s) {
    const size_t R = (size_t)a.N * (size_t)a.T;
    VSL_LAUNCH(k_window_gather, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, s, a);
}

}  // namespace vsl
