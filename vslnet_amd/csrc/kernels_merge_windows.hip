// Cross-window merge of top-K candidate lists (gfx950): the K_out best moments of every GROUP of lists in the video's own clip coordinates, with
// temporal non-maximum suppression ACROSS the lists (include/vslnet_hip.h, vsl_merge_windows).  A list is what vsl_extract_topk leaves for one
// (window, query) pair at window-local indices, a group is every window of one (query, video) pair: overlapping windows report the same moment twice,
// so the merge shifts every span by its window's offset and suppresses against what the group has already chosen.  The order is a strict total order on
// (key, global start, global end, list, slot) and suppression is a pure function of the chosen spans: the same bits on every run, nothing here is
// atomic.  The plan of k_merge_topk (kernels_merge.hip): one 256-thread workgroup per group, cached per-thread heads, no workspace, one launch.
#include "common.hpp"
#include "launch.hpp"

namespace vsl {

struct WinCand {
    float key;
    int s, e, list, slot;                    // global span ; list < 0: no candidate
};

// a strictly in front of b: key descending, then global start, global end, list and slot ascending.  Both are candidates.  (A NaN key is in front of
// nothing and nothing is in front of it: the choice is then unspecified, the loops stay bounded.)
__device__ __forceinline__ bool win_before(const WinCand& a, const WinCand& b) {
    if (a.key != b.key) return a.key > b.key;
    if (a.s != b.s) return a.s < b.s;
    if (a.e != b.e) return a.e < b.e;
    if (a.list != b.list) return a.list < b.list;
    return a.slot < b.slot;
}

__device__ __forceinline__ bool win_better(const WinCand& a, const WinCand& b) {
    return a.list >= 0 && (b.list < 0 || win_before(a, b));
}

// (s, e) against a chosen (cs, ce), clips [s, e + 1): suppressed iff the spans are identical -- at every nms_iou, so a duplicate from two windows is
// never reported twice -- or by k_extract_topk's rule: inter > 0 && (float)inter > nms_iou * (float)uni, the integers exact in fp32, ONE fp32 multiply
__device__ __forceinline__ bool win_suppressed(int s, int e, int cs, int ce, float nms_iou) {
    if (s == cs && e == ce) return true;
    const int inter = min(e, ce) - max(s, cs) + 1;
    const int uni = (e - s + 1) + (ce - cs + 1) - inter;
    return inter > 0 && (float)inter > nms_iou * (float)uni;
}

// The first candidate, in that order, of this thread's lists (tid, tid + 256, ... of group g) that none of the nch chosen spans suppresses.  Every
// candidate in front of the last choice has been chosen (and suppresses itself) or was suppressed when it was passed over, and suppression only
// grows: the scan needs no "behind the previous choice" condition.
__device__ __forceinline__ WinCand win_scan(const MergeWindowsArgs& a, int g, int tid, const int* chosen, int nch) {
    WinCand best{0.f, 0, 0, -1, 0};
    for (int b = tid; b < a.B; b += 256) {
        if (a.group_index[b] != g) continue;
        const int n = min(a.count[b], a.K);                     // (a negative count: no slot)
        const int off = a.offset ? a.offset[b] : 0;
        for (int slot = 0; slot < n; ++slot) {
            const size_t o = (size_t)b * a.K + slot;
            const WinCand c{a.key[o], (int)a.start[o] + off, (int)a.end[o] + off, b, slot};
            if (best.list >= 0 && !win_before(c, best)) continue;
            bool live = true;
            for (int q = 0; q < nch; ++q)                       // (chosen[] reads are wave-uniform addresses: LDS broadcasts)
                if (win_suppressed(c.s, c.e, chosen[2 * q], chosen[2 * q + 1], a.nms_iou)) { live = false; break; }
            if (live) best = c;
        }
    }
    return best;
}

// One workgroup of 256 threads per group.  Every thread holds the first live candidate of its own lists (its head); a block-wide argmin over the heads
// is the round's choice, which joins the chosen set in LDS (at most 32 spans).  Behind a round a thread looks for its next head when its head was
// taken OR is now suppressed by the new choice -- every other head is still live and still the first of its thread.  rescan_all (a measuring switch):
// every thread rescans every round, the scheme without the cached head.  Every loop is bounded by B, K and K_out.
__global__ __launch_bounds__(256) void k_merge_windows(MergeWindowsArgs a) {
    __shared__ WinCand red[4];
    __shared__ int chosen[2 * TOPK_MAX_K];
    const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, K_out = a.K_out;
    WinCand head = win_scan(a, g, tid, chosen, 0);
    int r = 0;
    for (; r < K_out; ++r) {
        WinCand m = head;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const WinCand o{__shfl_xor(m.key, x), __shfl_xor(m.s, x), __shfl_xor(m.e, x), __shfl_xor(m.list, x), __shfl_xor(m.slot, x)};
            if (win_better(o, m)) m = o;
        }
        __syncthreads();                                        // (everyone has read the previous round's winners)
        if (lane == 0) red[w] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (win_better(red[q], m)) m = red[q];
        if (m.list < 0) break;                                  // (block-uniform: every thread reduced the same four entries) the group is exhausted
        if (tid == 0) {
            const size_t o = (size_t)g * K_out + r;
            a.out_list[o] = m.list;
            a.out_start[o] = m.s;
            a.out_end[o] = m.e;
            a.out_score[o] = a.score[(size_t)m.list * a.K + m.slot];
            a.out_key[o] = m.key;
            chosen[2 * r] = m.s;
            chosen[2 * r + 1] = m.e;
        }
        if (r + 1 == K_out) continue;                           // (block-uniform) the last round needs no successor
        __syncthreads();                                        // (the new choice is in the chosen set)
        if (a.rescan_all || (head.list >= 0 && win_suppressed(head.s, head.e, m.s, m.e, a.nms_iou))) head = win_scan(a, g, tid, chosen, r + 1);
    }
    if (tid == 0) a.out_count[g] = r;
    for (int k = r + tid; k < K_out; k += 256) {                // slots from count on: -1, -1, -1, -inf, 0 (as k_merge_topk fills them)
        const size_t o = (size_t)g * K_out + k;
        a.out_list[o] = -1;
        a.out_start[o] = -1;
        a.out_end[o] = -1;
        a.out_score[o] = -INFINITY;
        a.out_key[o] = 0.f;
    }
}

void launch_merge_windows(const MergeWindowsArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_merge_windows, dim3(a.G), dim3(256), 0, s, a);
}

}  // namespace vsl
