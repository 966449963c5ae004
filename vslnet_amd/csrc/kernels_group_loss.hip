// The grouped training loss (gfx950; include/vslnet_hip.h, vsl_group_loss): vsl_loss's span and highlight losses over B pair rows cut into G groups
// -- one true (query, video) pair per group, its other rows the same query against other videos -- plus a softmax ranking term over every group's
// video relevances.  Nothing of the loss is defined here: the log-sum-exps, the per-element terms, the seeds and the batch sums are tile_bodies.hpp's
// (loss_sample_lse, loss_hl_term, loss_ce_seed, loss_hl_seed, loss_store: what k_loss_a / k_loss_c of kernels_head.hip are made of) and the relevance
// is rank_reduce.hpp's (what k_pair_relevance computes at search time).  No atomic anywhere: per-row partials go through the caller's scratch and
// are re-reduced in index order, so two runs give the same bits.
//   scratch layout (B floats / ints each): [0] lse_s | [1] lse_e | [2] ce (0 on a non-positive row) | [3] hl numerator | [4] mask sum |
//                                          [5] relevance r | [6] int: first valid clip at the maximum | [7] int: valid clips | [8] int: group of the row |
//                                          [9] z = r * inv_t.  z goes through MEMORY on purpose: formed where it is used, `r * inv_t - m` contracts into one fma
//                                          on the exact product, and a group of one no longer gets expf(0), l = 0 and d r = 0 exactly
#include "common.hpp"
#include "launch.hpp"
#include "rank_reduce.hpp"
#include "tile_bodies.hpp"

namespace vsl {

// group g's rows [gs, ge) and its positive row p, clamped so that every loop over them is bounded by B whatever the tables hold (p = -1: none)
__device__ __forceinline__ void group_rows(const GroupLossArgs& a, int g, int& gs, int& ge, int& p) {
    gs = min(max(a.group_start[g], 0), a.B);
    ge = min(max(a.group_start[g + 1], gs), a.B);
    p = a.positive[g];
    if (p < gs || p >= ge) p = -1;
}
__device__ __forceinline__ bool rank_finite(float z) { return z > -INFINITY && z < INFINITY; }      // (false for a NaN)
// the log-sum-exp of group [gs, ge) over its rows with a finite z, added in ascending row; false: the group is skipped (its positive row has no
// valid clip).  One thread; a caller whose threads all ask for the same group gets the same bits in each.
__device__ __forceinline__ bool group_lse(const float* __restrict__ z_, int gs, int ge, int p, float& lse) {
    if (p < 0 || !rank_finite(z_[p])) return false;
    float m = -INFINITY;
    for (int b = gs; b < ge; ++b) {
        const float z = z_[b];
        if (rank_finite(z)) m = fmaxf(m, z);
    }
    float ss = 0.f;
    for (int b = gs; b < ge; ++b) {
        const float z = z_[b];
        if (rank_finite(z)) ss += expf(z - m);
    }
    lse = m + logf(ss);
    return true;
}

// ---- k_group_loss_a: one 256-thread workgroup per row.  The row's group by a bisection of group_start (at most 32 steps); on a POSITIVE row the two
// log-sum-exps and the CE term (k_loss_a's expressions; a non-positive row reads neither its logits nor its labels); the highlight partials over
// every row; wave 0 reduces the relevance as k_pair_relevance does and finds the first valid clip that attains the maximum.
__global__ __launch_bounds__(256) void k_group_loss_a(GroupLossArgs a) {
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x, B = a.B, T = a.T;
    int lo = 0, hi = a.G;
    while (hi - lo > 1) {                                       // (block-uniform)
        const int mid = (lo + hi) >> 1;
        if (a.group_start[mid] <= b) lo = mid; else hi = mid;
    }
    const int g = lo;
    const bool pos = a.positive[g] == b;
    const float* s = a.sl + (size_t)b * T;
    const float* e = a.el + (size_t)b * T;
    const float* h = a.h + (size_t)b * T;
    const float* vm = a.vmask + (size_t)b * T;
    float lses = 0.f, lsee = 0.f, ce = 0.f;
    if (pos && a.s_lab) {                                       // (block-uniform)
        lses = loss_sample_lse(s, T, red);
        lsee = loss_sample_lse(e, T, red);
        ce = (lses - s[a.s_lab[b]]) + (lsee - e[a.e_lab[b]]);
    }
    float num = 0.f, den = 0.f;
    for (int t = tid; t < T; t += 256) {
        const float m = vm[t];
        if (a.h_lab) num += loss_hl_term(h[t], (float)a.h_lab[(size_t)b * T + t], m);
        den += m;
    }
    num = block_reduce(num, red, false);
    den = block_reduce(den, red, false);
    int* si = reinterpret_cast<int*>(a.scratch);
    if (tid < 64) {                                             // (wave 0; no barrier from here on)
        float best, sum;
        int cnt;
        pair_row_reduce(h, vm, T, tid, best, sum, cnt);
        int first = T;                                          // (a NaN maximum equals nothing: no clip, no rank gradient)
        for (int t = tid; t < T; t += 64)
            if (vm[t] != 0.f && h[t] == best) { first = t; break; }
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) first = min(first, __shfl_xor(first, x));
        if (tid == 0) {
            const float r = pair_row_relevance(best, sum, cnt, a.mean);
            a.scratch[5 * (size_t)B + b] = r;
            a.scratch[9 * (size_t)B + b] = r * a.inv_t;
            si[6 * (size_t)B + b] = first;
            si[7 * (size_t)B + b] = cnt;
            si[8 * (size_t)B + b] = g;
            if (a.pair_relevance) a.pair_relevance[b] = r;
            a.scratch[b] = lses;
            a.scratch[(size_t)B + b] = lsee;
            a.scratch[2 * (size_t)B + b] = ce;
            a.scratch[3 * (size_t)B + b] = num;
            a.scratch[4 * (size_t)B + b] = den;
        }
    }
}

// ---- k_group_loss_c: a (ceil(T / 256), B) grid writes the seeds; block (0, 0) the loss values and the hits.  Every block re-reduces the B per-row
// partials itself, as k_loss_c does (the same loops, the same tree: with every group of size one the sums are k_loss_c's bits), and every thread of
// a block forms its own group's log-sum-exp from the group's relevances.
__global__ __launch_bounds__(256) void k_group_loss_c(GroupLossArgs a) {
    __shared__ float red[8];
    __shared__ float lg[256];
    __shared__ int flag[256];
    const int B = a.B, T = a.T, tid = threadIdx.x;
    const float* scratch = a.scratch;
    const int* si = reinterpret_cast<const int*>(a.scratch);
    const float* z_ = scratch + 9 * (size_t)B;
    float ce = 0.f, num = 0.f, den = 0.f;
    for (int bb = tid; bb < B; bb += 256) { ce += scratch[2 * (size_t)B + bb]; num += scratch[3 * (size_t)B + bb]; den += scratch[4 * (size_t)B + bb]; }
    ce = block_reduce(ce, red, false);
    num = block_reduce(num, red, false);
    den = block_reduce(den, red, false);
    const float dsum = a.mask_sum > 0.f ? a.mask_sum : den;
    if (blockIdx.x == 0 && blockIdx.y == 0) {                   // (block-uniform)
        // thread t owns groups t, t + 256, ... of a chunk of 256: l_g = lse_g - z_pos and the hit; thread 0 adds a chunk's terms in ascending g
        float rank = 0.f;
        int hits = 0;
        for (int base = 0; base < a.G; base += 256) {
            const int g = base + tid;
            float l = 0.f;
            int f = 0;                                          // bit 0: the group counts; bit 1: its positive row ranks first
            if (g < a.G) {
                int gs, ge, p;
                group_rows(a, g, gs, ge, p);
                float lse;
                if (group_lse(z_, gs, ge, p, lse)) {
                    const float zp = z_[p];
                    l = lse - zp;
                    f = 3;
                    for (int bb = gs; bb < ge; ++bb) {          // order: z descending, then the smaller row
                        const float z = z_[bb];
                        if (bb != p && rank_finite(z) && (z > zp || (z == zp && bb < p))) f = 1;
                    }
                }
            }
            lg[tid] = l;
            flag[tid] = f;
            __syncthreads();
            if (tid == 0)
                for (int i = 0; i < min(256, a.G - base); ++i) {
                    if (flag[i] & 1) rank += lg[i];
                    hits += flag[i] >> 1;
                }
            __syncthreads();
        }
        if (tid == 0) {
            float four[4];
            loss_store(four, ce, num, dsum, a.inv_pos, a.w_loc, a.w_hl);
            const float rk = a.inv_groups * rank;
            a.losses[0] = four[0]; a.losses[1] = four[1]; a.losses[2] = rk; a.losses[3] = four[2] + a.w_rank * rk; a.losses[4] = four[3];
            if (a.hits) *a.hits = hits;
        }
    }
    if (!a.d_h) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + tid;
    if (t >= T) return;
    const int g = min(max(si[8 * (size_t)B + b], 0), a.G - 1);
    int gs, ge, p;
    group_rows(a, g, gs, ge, p);
    float dr = 0.f, lse;                                        // d total / d r_b
    if (b >= gs && b < ge && rank_finite(z_[b]) && group_lse(z_, gs, ge, p, lse))
        dr = a.w_rank * a.inv_groups * a.inv_t * (expf(z_[b] - lse) - (b == p ? 1.f : 0.f));
    const size_t i = (size_t)b * T + t;
    const float m = a.vmask[i];
    float dh = a.h_lab ? loss_hl_seed(a.h[i], (float)a.h_lab[i], m, a.w_hl, dsum) : 0.f;
    if (a.mean) { if (m != 0.f) dh += dr / (float)si[7 * (size_t)B + b]; }
    else if (t == si[6 * (size_t)B + b]) dh += dr;
    a.d_h[i] = dh;
    const bool pos = b == p && a.s_lab;
    const float cs = a.w_loc * a.inv_pos;
    a.d_sl[i] = pos ? loss_ce_seed(a.sl[i], scratch[b], t, (int)a.s_lab[b], cs) : 0.f;
    a.d_el[i] = pos ? loss_ce_seed(a.el[i], scratch[(size_t)B + b], t, (int)a.e_lab[b], cs) : 0.f;
}

void launch_group_loss_a(const GroupLossArgs& a, hipStream_t s) {
    VSL_LAUNCH(k_group_loss_a, dim3(a.B), dim3(256), 0, s, a);
}
void launch_group_loss_c(const GroupLossArgs& a, hipStream_t s) {
    const dim3 grid = a.d_h ? dim3((a.T + 255) / 256, a.B) : dim3(1, 1);       // (without seeds: the block that writes the loss values alone)
    VSL_LAUNCH(k_group_loss_c, grid, dim3(256), 0, s, a);
}

}  // namespace vsl
