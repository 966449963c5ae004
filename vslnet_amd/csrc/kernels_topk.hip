// Top-K moments per query (gfx950): greedy selection with temporal non-maximum suppression over the spans (s, e), 0 <= s <= e < L, of one sample,
// ranked by the logit sum sl[s] + el[e] (include/vslnet_hip.h, vsl_extract_topk).  softmax(sl)[s] * softmax(el)[e] = exp(sum - lse_s - lse_e) and the
// two normalisers are constant per sample: ranking by the sum is ranking by the joint probability of extract_index (layers_t7.py:355-363), and one
// IEEE addition is the same bits on every machine -- the search needs no exp and is exactly reproducible.  No (B, T, T) tensor, no workspace.
#include "common.hpp"
#include "launch.hpp"

namespace vsl {

constexpr int TOPK_NONE = 0xFFFF;            // "no live candidate" in the uint16 row cache (an end index is < MAX_L = 4096)
constexpr int TOPK_NO_ROW = 0x7fffffff;

// candidate (s, e) against a chosen (cs, ce), clips [s, e + 1): suppressed iff inter > 0 && (float)inter > nms_iou * (float)uni.  The integers are exact
// in fp32, there is ONE fp32 multiply.  A span suppresses itself only below nms_iou = 1, so the caller tests identity as well.
__device__ __forceinline__ bool topk_suppressed(int s, int e, int cs, int ce, float nms_iou) {
    const int inter = min(e, ce) - max(s, cs) + 1;
    const int uni = (e - s + 1) + (ce - cs + 1) - inter;
    return inter > 0 && (float)inter > nms_iou * (float)uni;
}

// order of the search: score descending, then the smaller row.  A row without a candidate loses to every row.
__device__ __forceinline__ bool topk_better(float sa, int ra, float sb, int rb) {
    return ra != TOPK_NO_ROW && (rb == TOPK_NO_ROW || sa > sb || (sa == sb && ra < rb));
}

// the first candidate in order (score descending, end ascending) of start row i that is neither chosen nor suppressed by one of the nch chosen spans:
// ends i .. hi - 1.  -> its end, or TOPK_NONE
__device__ __forceinline__ int topk_scan_row(const float* el, float si, int i, int hi, const int* chosen, int nch, float nms_iou) {
    float best = 0.f;
    int bj = TOPK_NONE;
    for (int j = i; j < hi; ++j) {
        const float v = si + el[j];
        if (bj != TOPK_NONE && !(v > best)) continue;          // (strict: the first maximal end stays)
        bool live = true;
        for (int c = 0; c < nch; ++c) {                        // (chosen[] reads are wave-uniform addresses: LDS broadcasts)
            const int cs = chosen[2 * c], ce = chosen[2 * c + 1];
            if ((cs == i && ce == j) || topk_suppressed(i, j, cs, ce, nms_iou)) { live = false; break; }
        }
        if (live) { best = v; bj = j; }
    }
    return bj;
}

// log-sum-exp of T logits held in LDS by the 256-thread workgroup: max, then the sum of expf, as k_extract_index normalises (every thread gets the result)
__device__ __forceinline__ float topk_lse(const float* x, int T, float* red) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float mx = -3.0e38f;
    for (int t = tid; t < T; t += 256) mx = fmaxf(mx, x[t]);
    mx = wave_max(mx);
    __syncthreads();
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float ss = 0.f;
    for (int t = tid; t < T; t += 256) ss += expf(x[t] - mx);
    ss = wave_sum(ss);
    __syncthreads();
    if (lane == 0) red[w] = ss;
    __syncthreads();
    return mx + logf(((red[0] + red[1]) + red[2]) + red[3]);
}

// One workgroup per sample.  LDS: sl, el (T floats each), rowend[T] uint16 = the end of the first-in-order LIVE candidate of start row i (its score is
// sl[i] + el[rowend[i]], recomputed: one addition), the chosen spans and reduction scratch: 10 T + 304 bytes, 40.3 KiB at T = 4096.
//   round 0: thread tid fills rows tid, tid + 256, ... (the interleaving balances the triangular row lengths); a block argmax over the rows picks choice 0;
//   round r: a row's cached candidate stays the row's first live one unless it IS the new choice or the new choice suppresses it -- only such rows
//            (necessarily rows <= the chosen end) are rescanned, each end tested against the r + 1 chosen spans; then the block argmax again.
// Every loop is bounded by K and T: NaN logits give an unspecified choice, never a hang.
__global__ __launch_bounds__(256) void k_extract_topk(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
    const int T = a.T, K = a.K;
    float* sl = reinterpret_cast<float*>(topk_smem);
    float* el = sl + T;
    int* chosen = reinterpret_cast<int*>(el + T);               // [32][2]
    float* red_s = reinterpret_cast<float*>(chosen + 64);       // [4] wave winners: score
    int* red_r = reinterpret_cast<int*>(red_s + 4);             // [4] ... row
    float* red = reinterpret_cast<float*>(red_r + 4);           // [4] log-sum-exp scratch
    uint16_t* rowend = reinterpret_cast<uint16_t*>(red + 4);    // [T]
    const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int t = tid; t < T; t += 256) {
        sl[t] = a.sl[(size_t)b * T + t];
        el[t] = a.el[(size_t)b * T + t];
    }
    __syncthreads();
    float lse_s = 0.f, lse_e = 0.f;
    if (a.prob) {                                               // (block-uniform) over the sample's T logits, as the reference's softmax runs
        lse_s = topk_lse(sl, T, red);
        lse_e = topk_lse(el, T, red);
    }
    const int L = a.valid_len ? min(max(a.valid_len[b], 1), T) : T;
    const int span = a.max_span > 0 && a.max_span < T ? a.max_span : T;      // (clamped: i + span stays far from INT_MAX for every legal max_span)
    for (int i = tid; i < L; i += 256) rowend[i] = (uint16_t)topk_scan_row(el, sl[i], i, min(L, i + span), chosen, 0, a.nms_iou);
    __syncthreads();
    int r = 0;
    for (; r < K; ++r) {
        float bs = 0.f;
        int br = TOPK_NO_ROW;
        for (int i = tid; i < L; i += 256) {                    // rows ascending: strict > keeps the smaller row
            const int j = rowend[i];
            if (j == TOPK_NONE) continue;
            const float v = sl[i] + el[j];
            if (br == TOPK_NO_ROW || v > bs) { bs = v; br = i; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float os = __shfl_xor(bs, m);
            const int orow = __shfl_xor(br, m);
            if (topk_better(os, orow, bs, br)) { bs = os; br = orow; }
        }
        if (lane == 0) { red_s[w] = bs; red_r[w] = br; }
        __syncthreads();
        bs = red_s[0]; br = red_r[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (topk_better(red_s[q], red_r[q], bs, br)) { bs = red_s[q]; br = red_r[q]; }
        if (br == TOPK_NO_ROW) break;                           // (block-uniform: every thread reduced the same four entries) no candidate is left
        const int ce = rowend[br];
        if (tid == 0) {
            const size_t o = (size_t)b * K + r;
            a.start_index[o] = br;
            a.end_index[o] = ce;
            a.score[o] = bs;
            if (a.prob) a.prob[o] = expf(bs - lse_s - lse_e);
            chosen[2 * r] = br;
            chosen[2 * r + 1] = ce;
        }
        __syncthreads();                                        // the choice is in LDS; everyone has read rowend[br] and the wave winners
        if (r + 1 == K) continue;                               // (block-uniform) the last round needs no new candidates
        for (int i = tid; i <= ce; i += 256) {
            const int j = rowend[i];
            if (j == TOPK_NONE) continue;
            if ((i == br && j == ce) || topk_suppressed(i, j, br, ce, a.nms_iou))
                rowend[i] = (uint16_t)topk_scan_row(el, sl[i], i, min(L, i + span), chosen, r + 1, a.nms_iou);
        }
        __syncthreads();
    }
    if (tid == 0 && a.count) a.count[b] = r;
    for (int k = r + tid; k < K; k += 256) {                    // slots from count on: -1, -1, -inf, 0
        const size_t o = (size_t)b * K + k;
        a.start_index[o] = -1;
        a.end_index[o] = -1;
        a.score[o] = -INFINITY;
        if (a.prob) a.prob[o] = 0.f;
    }
}

size_t extract_topk_lds_bytes(int T) { return (size_t)T * 10 + (64 + 12) * sizeof(int); }

void launch_extract_topk(const TopkArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_extract_topk, dim3(a.B), dim3(256), extract_topk_lds_bytes(a.T), s, a);
}

}  // namespace vsl
