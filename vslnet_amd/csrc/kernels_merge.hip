// Cross-list merge of top-K candidate lists (gfx950): the K_out best candidates of every GROUP of lists (include/vslnet_hip.h, vsl_merge_topk).  A list is
// what vsl_extract_topk leaves for one (query, video) pair -- K slots, `count` of them filled -- a group is every list of one query: the merge turns
// per-pair top-K lists into one ranked list per query without a (B, K) copy to the host.  The order is a strict total order on (key, tag, list, slot):
// a round's choice is a pure function of the inputs, so the result is the same bits on every run and nothing here is atomic.  No workspace.
#include "common.hpp"
#include "launch.hpp"

namespace vsl {

struct MergeCand {
    float key;
    int tag, list, slot;                     // list < 0: no candidate
};

// a strictly in front of b: key descending, then tag, list and slot ascending.  Both are candidates.  (A NaN key is in front of nothing and nothing is in
// front of it: it can be a round's choice only when the round has no other, and then it ends the search.)
__device__ __forceinline__ bool merge_before(const MergeCand& a, const MergeCand& b) {
    if (a.key != b.key) return a.key > b.key;
    if (a.tag != b.tag) return a.tag < b.tag;
    if (a.list != b.list) return a.list < b.list;
    return a.slot < b.slot;
}

__device__ __forceinline__ bool merge_better(const MergeCand& a, const MergeCand& b) {
    return a.list >= 0 && (b.list < 0 || merge_before(a, b));
}

// the first candidate, in that order, of this thread's lists (tid, tid + 256, ... of group g) that is strictly behind `prev` (have_prev = false: the first)
__device__ __forceinline__ MergeCand merge_scan(const MergeArgs& a, int g, int tid, const MergeCand& prev, bool have_prev) {
    MergeCand best{0.f, 0, -1, 0};
    for (int b = tid; b < a.B; b += 256) {
        if (a.group_index[b] != g) continue;
        const int n = min(a.count[b], a.K);                     // (a negative count: no slot)
        const int list_tag = a.tag && !a.tag_per_slot ? a.tag[b] : b;
        for (int slot = 0; slot < n; ++slot) {
            const size_t o = (size_t)b * a.K + slot;
            const MergeCand c{a.key[o], a.tag_per_slot ? a.tag[o] : list_tag, b, slot};
            if (have_prev && !merge_before(prev, c)) continue;
            if (merge_better(c, best)) best = c;
        }
    }
    return best;
}

// One workgroup of 256 threads per group.  Round r selects the successor of round r - 1's choice: every thread holds the first candidate of its own
// lists behind the previous choice (its head), a block-wide argmin over the heads is the round's choice, and only the thread whose head was taken
// looks for its next one -- every other head is still behind the new choice and still the first of its thread.  No per-list cursor, no LDS beyond
// the four wave winners.  rescan_all (a measuring switch): every thread rescans every round, the scheme without the cached head.
// Every loop is bounded by B, K and K_out.
__global__ __launch_bounds__(256) void k_merge_topk(MergeArgs a) {
    __shared__ MergeCand red[4];
    const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, K_out = a.K_out;
    MergeCand head = merge_scan(a, g, tid, MergeCand{0.f, 0, -1, 0}, false);
    int r = 0;
    for (; r < K_out; ++r) {
        MergeCand m = head;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const MergeCand o{__shfl_xor(m.key, x), __shfl_xor(m.tag, x), __shfl_xor(m.list, x), __shfl_xor(m.slot, x)};
            if (merge_better(o, m)) m = o;
        }
        __syncthreads();                                        // (everyone has read the previous round's winners)
        if (lane == 0) red[w] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (merge_better(red[q], m)) m = red[q];
        if (m.list < 0) break;                                  // (block-uniform: every thread reduced the same four entries) the group is exhausted
        if (tid == 0) {
            const size_t o = (size_t)g * K_out + r, i = (size_t)m.list * a.K + m.slot;
            a.out_tag[o] = m.tag;
            a.out_list[o] = m.list;
            a.out_start[o] = a.start[i];
            a.out_end[o] = a.end[i];
            a.out_score[o] = a.score[i];
            a.out_key[o] = m.key;
        }
        if (r + 1 == K_out) continue;                           // (block-uniform) the last round needs no successor
        if (a.rescan_all || (head.list == m.list && head.slot == m.slot)) head = merge_scan(a, g, tid, m, true);
    }
    if (tid == 0) a.out_count[g] = r;
    for (int k = r + tid; k < K_out; k += 256) {                // slots from count on: -1, -1, -1, -1, -inf, 0
        const size_t o = (size_t)g * K_out + k;
        a.out_tag[o] = -1;
        a.out_list[o] = -1;
        a.out_start[o] = -1;
        a.out_end[o] = -1;
        a.out_score[o] = -INFINITY;
        a.out_key[o] = 0.f;
    }
}

void launch_merge_topk(const MergeArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_merge_topk, dim3(a.G), dim3(256), 0, s, a);
}

}  // namespace vsl
