// The attention core's shared device parts and the launcher contract between its units (kernels_attn.hip: dispatch + query-major dQ;
// kernels_attn_h16.hip: 8 heads; kernels_attn_hd.hip: 4 / 16 heads; kernels_attn_wide.hip: 1 / 2 heads).  Included by those units only:
// everything else sees AttnArgs, launch_attn_fwd / launch_attn_bwd and the slab counts of launch.hpp.
//   a8 (:174-182)  S = Q K^T / sqrt(hd) + (1 - mask[key]) * -1e30 ; P = softmax ; O = drop(P) V
#pragma once
#include "common.hpp"
#include "launch.hpp"
#include <type_traits>

namespace vsl {

constexpr float ATTN_LOG2E = 1.4426950408889634f, ATTN_LN2 = 0.6931471805599453f;

template <int HDV> struct AttnHead {
    static_assert(HDV == 8 || HDV == 16 || HDV == 32 || HDV == 64 || HDV == 128, "head sizes of num_heads 16, 8, 4, 2, 1");
    static constexpr float scale = HDV == 128 ? 0.08838834764831845f : HDV == 64 ? 0.125f : HDV == 32 ? 0.17677669529663687f     // 1 / sqrt(hd)
                                 : HDV == 16 ? 0.25f : 0.35355339059327373f;
    static constexpr int NC = HDV / 4;                  // head dims a lane contributes to a score tile: k group g owns dims g NC .. g NC + NC - 1
    static constexpr int NT = HDV >= 16 ? HDV / 16 : 1; // 16-row tiles of the head dims in the value-side products (hd 8: half a tile)
    static constexpr int KST = HDV + 4;                 // LDS row stride of a head slice
    static constexpr int F4 = HDV / 4;                  // float4 per head-slice row
};

// N consecutive floats into registers (16-byte aligned for N >= 4, 8-byte for N = 2)
template <int N> __device__ __forceinline__ void load_nc(const float* p, float* out) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + i);
            out[i] = v.x; out[i + 1] = v.y; out[i + 2] = v.z; out[i + 3] = v.w;
        }
    } else {
        static_assert(N == 2, "");
        const float2 v = *reinterpret_cast<const float2*>(p);
        out[0] = v.x; out[1] = v.y;
    }
}
template <int N> __device__ __forceinline__ void zero_nc(float* out) {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = 0.f;
}
// additive key bias (natural-log units) of key k0 + t of the sample whose mask row starts at mask[rowbase]; a pad key past L carries the mask value
__device__ __forceinline__ float attn_key_bias(const float* mask, size_t rowbase, int k0, int t, int L) {
    return k0 + t < L ? (1.0f - mask[rowbase + k0 + t]) * MASK_VALUE : MASK_VALUE;
}

// ---------------------------------------------------------------------------------------------------------
// Dropout of the probabilities (d2).  The forward and every backward must draw the same decision for (query row, key), where
// qrow = ((b + b_off) H + h) L + q counts the (sample, head, query) rows of the whole batch:
//   L <= 256  (PAIR = false): one hash per element, drop_hash(qrow * L + key);
//   L  > 256  (PAIR = true) : one hash per key pair, h = drop_hash(qrow * ceil(L / 2) + key / 2); the even key compares h, the odd key drop_hash_odd(h).
// keep = hash >= d2.thresh, multiplier d2.scale or 0.  tests/helpers.py (hip_dropout) restates it.  All index arithmetic is 32-bit and wraps.
// The index formulas and the pair decode below are the only statement of that contract on the device.  (The element form's loop over a lane's four
// registers stays in the streamed kernels: a loop inside a helper is unrolled and folded before the kernel's own loops are, and their code depends on it.)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t attn_drop_elem(uint32_t qrow, int L, int key) { return qrow * (uint32_t)L + (uint32_t)key; }
__device__ __forceinline__ uint32_t attn_drop_pair_stride(int L) { return (uint32_t)((L + 1) >> 1); }
__device__ __forceinline__ uint32_t attn_drop_pair_row(uint32_t qrow, int L) { return qrow * attn_drop_pair_stride(L); }     // + key / 2 = the pair's index
__device__ __forceinline__ float attn_drop_pair_mul(const Drop& d2, int odd, uint32_t h) {       // h: the pair's hash, odd: which key of the pair
    return (odd ? drop_hash_odd(h) : h) >= d2.thresh ? d2.scale : 0.f;
}
// query-major, pair form: one query row (prow = attn_drop_pair_row), the four consecutive keys k4 .. k4 + 3 (k4 a multiple of 4: two whole pairs);
// v[r] <- v[r] * multiplier.  The caller has tested d2.thresh != 0.
__device__ __forceinline__ void attn_drop_pair4(const Drop& d2, uint32_t prow, int k4, float* v) {
    const uint32_t pi = prow + (uint32_t)(k4 >> 1);
    const uint32_t h0 = drop_hash(pi, d2.seed, d2.key), h1 = drop_hash(pi + 1u, d2.seed, d2.key);
    v[0] = h0 >= d2.thresh ? v[0] * d2.scale : 0.f;
    v[1] = drop_hash_odd(h0) >= d2.thresh ? v[1] * d2.scale : 0.f;
    v[2] = h1 >= d2.thresh ? v[2] * d2.scale : 0.f;
    v[3] = drop_hash_odd(h1) >= d2.thresh ? v[3] * d2.scale : 0.f;
}
// query-major, either form: m2[r] <- multiplier of (qrow, k4 + r), 1 with dropout off
template <bool PAIR> __device__ __forceinline__ void attn_drop_q4(const Drop& d2, uint32_t qrow, int L, int k4, float* m2) {
    if (d2.thresh == 0u) { m2[0] = m2[1] = m2[2] = m2[3] = 1.f; return; }
    if (!PAIR) {
        const uint32_t ei = attn_drop_elem(qrow, L, k4);
#pragma unroll
        for (int r = 0; r < 4; ++r) m2[r] = drop_keep_scale(d2, ei + r);
    } else {
        const uint32_t pi = attn_drop_pair_row(qrow, L) + (uint32_t)(k4 >> 1);
        const uint32_t h0 = drop_hash(pi, d2.seed, d2.key), h1 = drop_hash(pi + 1u, d2.seed, d2.key);
        m2[0] = attn_drop_pair_mul(d2, 0, h0); m2[1] = attn_drop_pair_mul(d2, 1, h0);
        m2[2] = attn_drop_pair_mul(d2, 0, h1); m2[3] = attn_drop_pair_mul(d2, 1, h1);
    }
}
// (key-major, pair form -- lane (ki, g) of a 16 x 16 tile holds one key and four queries: the lane and its neighbour, the other key of the pair, hash
// two queries each and exchange the words, then attn_drop_pair_mul(d2, ki & 1, .).  That block is spelled out in k_attn_bwd_long, k_attn_hd_bwd and
// k_attn_wide_dkv: every helper shape tried for it changed their code.)

// ---------------------------------------------------------------------------------------------------------
// host side: the choice of an instantiation, written once
// ---------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, hd>) for the head size hd = 128 / H, if it is one of HDS
template <int... HDS, class F> void attn_for_head_size(int H, F&& f) {
    const bool hit = ((H * HDS == D ? (f(std::integral_constant<int, HDS>{}), true) : false) || ...);
    if (!hit) {
        fprintf(stderr, "[vslnet_hip] num_heads=%d has no attention kernel\n", H);
        abort();
    }
}
template <class F> void attn_for_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
inline bool attn_pair_hash(int L) { return L > 256; }          // the probability site's keying (above)

// the per-family launchers behind launch_attn_fwd / launch_attn_bwd (kernels_attn.hip).  dq = false (L > ATTN_SLAB_MAX_L only): dK / dV alone,
// the key blocks write no dQ partials (k_attn_dq computes dQ); query_major: k_attn_wide_dq writes the complete dQ into slab 0
void launch_attn_h16_fwd(const AttnArgs& a, hipStream_t s);
void launch_attn_h16_bwd(const AttnArgs& a, bool dq, hipStream_t s);
void launch_attn_hd_fwd(const AttnArgs& a, hipStream_t s);
void launch_attn_hd_bwd(const AttnArgs& a, bool dq, hipStream_t s);
void launch_attn_wide_fwd(const AttnArgs& a, hipStream_t s);
void launch_attn_wide_bwd(const AttnArgs& a, bool query_major, hipStream_t s);
bool attn_dq_query_major(int L);

}  // namespace vsl
