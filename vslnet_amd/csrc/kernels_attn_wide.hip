// Attention core of num_heads 1 and 2 (head sizes 128 and 64), forward and backward, every L up to MAX_L.  The kernels of the other head
// counts: kernels_attn_hd.hip, kernels_attn_h16.hip, k_attn_dq; kernels_attn.hip routes H <= 2 here, L <= 128 included.
//   a8 (:174-182)  S = Q K^T / sqrt(hd) + (1 - mask[key]) * -1e30 ; P = softmax ; O = drop(P) V
// Same contracts as the other head counts: Q / K / V / att are (R, 128) rows with head h at columns h hd .. h hd + hd - 1, LSE is saved per
// (b, h, q) in natural-log units, and dQ leaves the backward as attn_dq_slabs(L) (R, 128) slabs that k_qkv_bwd adds: one partial per 256-key
// block up to ATTN_SLAB_MAX_L (or with VSL_ATTN_DQ_SLABS=1), the whole dQ in slab 0 above.  The probability dropout is keyed as for every
// other head count: one drop_hash per element for L <= 256, key pairs (drop_hash_odd, ceil(L / 2) hashes per row) above.
// Every product runs on the fp32-input MFMA (v_mfma_f32_16x16x4_f32): exact fp32 products, no split planes.
//
// Why these tiles.  At 1 or 2 heads a (query block, head, sample) grid is 2 / 4 x narrower than at 4 / 8 heads: 64-query workgroups would give
// configs[1] (B = 64, T = 128) 128 forward workgroups for 256 CUs.  So every kernel here is 16 rows (queries, or keys for dK / dV) by 4 waves,
// and the 4 waves split the OTHER sequence axis round-robin in 16-row tiles (configs[1], H = 1: 512 workgroups of 4 waves per kernel).  Each
// wave keeps its own partial (online-softmax state, dK / dV, dQ) in registers and the workgroup adds the 4 partials in LDS in wave order at the
// end: a fixed summation order, no atomics.  A K / V (or Q / dA) row then feeds exactly one wave, so nothing is staged in LDS for reuse: the
// score-tile operands (a lane's NC = hd / 4 consecutive dims of one row) and the value-side operands come straight from global memory (L2).
// The value-side products map row i of 16-row tile j to head dim NT i + j (NT = hd / 16), which makes a lane's operands NT consecutive floats
// (float4 loads) and its results NT consecutive dims of one row (float4 stores).  Registers: the head-dim accumulators (NT f32x4 = 32 at
// hd 128, two sets in dK / dV) and the NC-wide score operands (32 each), far below the 128-per-lane wall of the 1024-thread kernels.
#include "attn.hpp"

namespace vsl {

template <int HDV> struct AttnWide : AttnHead<HDV> {
    static_assert(HDV == 64 || HDV == 128, "head sizes 64 and 128");
    static constexpr int N4 = AttnHead<HDV>::NT / 4;    // float4 per lane of the NT dims of a value-side row (row i of tile j = head dim NT i + j)
    static constexpr int ST = AttnHead<HDV>::KST;       // LDS row stride of the wave partials
};

// the lane's accumulator rows 4 g + r of NT head-dim tiles -> row `dst` of an LDS partial: dims NT (4 g + r) + j
template <int NT> __device__ __forceinline__ void aw_park(const f32x4* acc, float* dst, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f = 0; f < NT / 4; ++f)
            *reinterpret_cast<float4*>(dst + NT * (4 * g + r) + 4 * f) = make_float4(acc[4 * f][r], acc[4 * f + 1][r], acc[4 * f + 2][r], acc[4 * f + 3][r]);
}
// ---------------------------------------------------------------------------------------------------------
// forward.  Workgroup = (16 queries, head, sample); wave w takes the key tiles 16 (4 i + w).  Lane (qi, g) owns query column qi of the
// transposed score tile S^T = K Q^T (keys 16 t + 4 g + r): the online softmax is lane-local up to two cross-group exchanges, in the log2 domain
// as in k_attn_fwd.  O^T += V^T P^T with A[i][k = g] = V[key 4 g + r][NT i + j], B = P^T straight from the score registers.  At the end the
// 4 wave states (max, sum, O) are merged in LDS in wave order.
// ---------------------------------------------------------------------------------------------------------
template <int HDV, bool PAIR>
__global__ __launch_bounds__(256) void k_attn_wide_fwd(const float* __restrict__ Q, const float* __restrict__ K,
                                                       const float* __restrict__ V, const float* __restrict__ mask,
                                                       float* __restrict__ att, float* __restrict__ lse, int L, int H,
                                                       int b_off, Drop d2) {
    using C = AttnWide<HDV>;
    constexpr int NC = C::NC, NT = C::NT, N4 = C::N4, ST = C::ST;
    __shared__ __attribute__((aligned(16))) float Os[4 * 16 * ST];    // [wave][query][dim] unnormalised partial O of each wave
    __shared__ float Ms[4 * 16], Ss[4 * 16];                          // [wave][query] running max (log2) and sum
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int qb, h, b;
    xcd_swizzle(qb, h, b);                         // grid (ceil(L / 16), H, B)
    const size_t rowbase = (size_t)b * L;
    const int qi = lane & 15, g = lane >> 4;
    const int q = qb * 16 + qi;
    const int Lp = (L + 15) & ~15;
    float qr[NC];                                  // B operand of S^T: Q[q][g NC + c]
    zero_nc<NC>(qr);
    if (q < L) load_nc<NC>(Q + (rowbase + q) * D + h * HDV + g * NC, qr);
    const float c2 = C::scale * ATTN_LOG2E;
    const uint32_t qrow = (uint32_t)(((size_t)(b + b_off) * H + h) * L + q);
    float m = -3.0e38f, l = 0.f;
    f32x4 o[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 16 * w; kt < Lp; kt += 64) {
        float kr[NC];                              // A operand of S^T: K[kt + qi][g NC + c]
        zero_nc<NC>(kr);
        if (kt + qi < L) load_nc<NC>(K + (rowbase + kt + qi) * D + h * HDV + g * NC, kr);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c], qr[c], s, 0, 0, 0);
        const int k4 = kt + 4 * g;                 // the lane's keys k4 .. k4 + 3
        float x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = fmaf(s[r], c2, attn_key_bias(mask, rowbase, 0, k4 + r, L) * ATTN_LOG2E);
        float tmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        tmax = lane_pair16(tmax, [](float a, float bb) { return fmaxf(a, bb); });
        tmax = lane_pair32(tmax, [](float a, float bb) { return fmaxf(a, bb); });
        const float mn = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[j][r] *= alpha;
        float pr[4], m2[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { pr[r] = __builtin_amdgcn_exp2f(x[r] - mn); l += pr[r]; }
        attn_drop_q4<PAIR>(d2, qrow, L, k4, m2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float vv[NT];                          // A operand: V[k4 + r][NT qi + j]
            zero_nc<NT>(vv);
            if (k4 + r < L) load_nc<NT>(V + (rowbase + k4 + r) * D + h * HDV + NT * qi, vv);
            const float pd = pr[r] * m2[r];
#pragma unroll
            for (int j = 0; j < NT; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[j], pd, o[j], 0, 0, 0);
        }
    }
    l = lane_pair16(l, [](float a, float bb) { return a + bb; });
    l = lane_pair32(l, [](float a, float bb) { return a + bb; });
    if (g == 0) { Ms[w * 16 + qi] = m; Ss[w * 16 + qi] = l; }
    aw_park<NT>(o, Os + (w * 16 + qi) * ST, g);    // lane (qi, g) holds O^T[NT (4 g + r) + j][qi]
    __syncthreads();
    // merge: thread (query cq, chunk cc) owns dims NT cc .. NT cc + NT - 1; wave order 0..3 everywhere
    const int cq = tid >> 4, cc = tid & 15, qo = qb * 16 + cq;
    if (qo < L) {
        const float M = fmaxf(fmaxf(Ms[cq], Ms[16 + cq]), fmaxf(Ms[32 + cq], Ms[48 + cq]));
        float wt[4], sum = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) { wt[v] = __builtin_amdgcn_exp2f(Ms[v * 16 + cq] - M); sum += wt[v] * Ss[v * 16 + cq]; }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int f = 0; f < N4; ++f) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 p = *reinterpret_cast<const float4*>(&Os[(v * 16 + cq) * ST + NT * cc + 4 * f]);
                a.x = fmaf(wt[v], p.x, a.x); a.y = fmaf(wt[v], p.y, a.y); a.z = fmaf(wt[v], p.z, a.z); a.w = fmaf(wt[v], p.w, a.w);
            }
            *reinterpret_cast<float4*>(att + (rowbase + qo) * D + h * HDV + NT * cc + 4 * f) = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
        }
        if (cc == 0 && lse) lse[((size_t)b * H + h) * L + qo] = M * ATTN_LN2 + __logf(sum);
    }
}

// ---------------------------------------------------------------------------------------------------------
// dK / dV.  Workgroup = (16 keys, head, sample); wave w takes the query tiles 16 (4 i + w).  Lane (ki, g) keeps K and V of key ki (its NC dims)
// in registers.  Per query tile: S = Q K^T and dP = dA V^T (A = the lane's Q / dA row slice, read from global memory and parked in the wave's
// LDS rows for the second layout), P = exp(S c + bias - LSE), the forward's dropout decisions (key pairs: the lane and its neighbour exchange
// hashes, as k_attn_bwd_long), dS = P (dP m2 - Delta) c, then dV^T += dA^T (P m2) and dK^T += Q^T dS with A[i][k = g] = dA / Q[q 4 g + r][NT i + j].
// Delta_q = dA . O is formed from the same row slices.  The 4 wave partials are added in LDS in wave order.
// ---------------------------------------------------------------------------------------------------------
template <int HDV> constexpr size_t attn_wide_dkv_lds() { return (size_t)(2 * 4 * 16 * AttnWide<HDV>::ST + 2 * 4 * 16) * sizeof(float); }

template <int HDV, bool PAIR>
__global__ __launch_bounds__(256) void k_attn_wide_dkv(const float* __restrict__ Q, const float* __restrict__ K,
                                                       const float* __restrict__ V, const float* __restrict__ att,
                                                       const float* __restrict__ dr, const float* __restrict__ lse,
                                                       const float* __restrict__ mask, float* __restrict__ dK,
                                                       float* __restrict__ dV, int L, int H, int b_off, Drop d2, Drop d3) {
    using C = AttnWide<HDV>;
    constexpr int NC = C::NC, NT = C::NT, N4 = C::N4, ST = C::ST;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;                              // [wave][16][ST] Q rows of the wave's query tile (then: the dK partials)
    float* As = Qs + 4 * 16 * ST;                  // [wave][16][ST] dA = dr * m3 rows (then: the dV partials)
    float* Ls = As + 4 * 16 * ST;                  // [wave][16] LSE
    float* Ds = Ls + 4 * 16;                       // [wave][16] Delta = dA . O
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int kb, h, b;
    xcd_swizzle(kb, h, b);                         // grid (ceil(L / 16), H, B)
    const size_t rowbase = (size_t)b * L;
    const int ki = lane & 15, g = lane >> 4;
    const int key = kb * 16 + ki;
    const int Lp = (L + 15) & ~15;
    float kr[NC], vr[NC];                          // B operands of S and dP: K[key][g NC + c], V[key][g NC + c]
    zero_nc<NC>(kr); zero_nc<NC>(vr);
    if (key < L) {
        load_nc<NC>(K + (rowbase + key) * D + h * HDV + g * NC, kr);
        load_nc<NC>(V + (rowbase + key) * D + h * HDV + g * NC, vr);
    }
    const float mbk = attn_key_bias(mask, rowbase, 0, key, L);
    const float scale = C::scale;
    const uint32_t hb = (uint32_t)(((size_t)(b + b_off) * H + h) * L);
    f32x4 dk[NT], dv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* Qw = Qs + w * 16 * ST;
    float* Aw = As + w * 16 * ST;
    float* Lw = Ls + w * 16;
    float* Dw = Ds + w * 16;
    const int nit = (Lp / 16 + 3) / 4;             // query tiles per wave, the same trip count in every wave (barriers)
    for (int it = 0; it < nit; ++it) {
        const int qt = 16 * (4 * it + w);
        const bool act = qt < Lp;
        const int qrow = qt + ki;
        float qa[NC], aa[NC];                      // A operands of S and dP: Q[qt + ki][g NC + c], dA[qt + ki][g NC + c]
        zero_nc<NC>(qa); zero_nc<NC>(aa);
        float dl = 0.f, lq = 0.f;
        if (act && qrow < L) {
            const size_t off = (rowbase + qrow) * D + h * HDV + g * NC;
            float oa[NC];
            load_nc<NC>(Q + off, qa);
            load_nc<NC>(dr + off, aa);
            load_nc<NC>(att + off, oa);
            if (d3.thresh) {                       // r = drop3(att) + x  (:183-184): element-keyed
#pragma unroll
                for (int c = 0; c < NC; ++c) aa[c] *= drop_keep_scale(d3, (uint32_t)(off + c));
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) dl = fmaf(aa[c], oa[c], dl);
            lq = lse[((size_t)b * H + h) * L + qrow];
        }
        dl += __shfl_xor(dl, 16);                  // the four k groups of the row in a fixed order
        dl += __shfl_xor(dl, 32);
        if (act) {
#pragma unroll
            for (int c = 0; c < NC; c += 4) {
                *reinterpret_cast<float4*>(&Qw[ki * ST + g * NC + c]) = make_float4(qa[c], qa[c + 1], qa[c + 2], qa[c + 3]);
                *reinterpret_cast<float4*>(&Aw[ki * ST + g * NC + c]) = make_float4(aa[c], aa[c + 1], aa[c + 2], aa[c + 3]);
            }
            if (g == 0) { Lw[ki] = lq; Dw[ki] = dl; }
        }
        __syncthreads();
        if (act) {
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[c], kr[c], sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[c], vr[c], dp, 0, 0, 0);
            }
            // lane (ki, g), register r: query qt + 4 g + r, key kb 16 + ki
            float m2v[4] = {1.f, 1.f, 1.f, 1.f};
            if (!PAIR) {
#pragma unroll
                for (int r = 0; r < 4; ++r) m2v[r] = drop_mul(d2, attn_drop_elem(hb + (uint32_t)(qt + 4 * g + r), L, key));
            } else if (d2.thresh != 0u) {          // keys 2 j, 2 j + 1 share a hash: this lane hashes two of the four queries, its neighbour the other two
                const uint32_t Lh = attn_drop_pair_stride(L), kp = (uint32_t)(key >> 1);
                const int odd = ki & 1;
                uint32_t hm[2], hp[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    hm[jj] = drop_hash((hb + (uint32_t)(qt + 4 * g + 2 * odd + jj)) * Lh + kp, d2.seed, d2.key);
                    hp[jj] = __float_as_uint(lane_xor1(__uint_as_float(hm[jj])));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) m2v[r] = attn_drop_pair_mul(d2, odd, (r >> 1) == odd ? hm[r & 1] : hp[r & 1]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 4 * g + r;
                const float p = __expf(sc[r] * scale + mbk - Lw[ql]);
                const float pd = p * m2v[r];
                const float ds = p * (dp[r] * m2v[r] - Dw[ql]) * scale;
                float av[NT], qv[NT];
                load_nc<NT>(&Aw[ql * ST + NT * ki], av);
                load_nc<NT>(&Qw[ql * ST + NT * ki], qv);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    dv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], pd, dv[j], 0, 0, 0);
                    dk[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[j], ds, dk[j], 0, 0, 0);
                }
            }
        }
        __syncthreads();                           // the wave's rows are read before the next tile overwrites them
    }
    aw_park<NT>(dk, Qs + (w * 16 + ki) * ST, g);   // lane (ki, g) holds dK^T / dV^T[NT (4 g + r) + j][ki]
    aw_park<NT>(dv, As + (w * 16 + ki) * ST, g);
    __syncthreads();
    const int ck = tid >> 4, cc = tid & 15, ko = kb * 16 + ck;
    if (ko < L) {
#pragma unroll
        for (int f = 0; f < N4; ++f) {
            const int col = NT * cc + 4 * f;
            float4 sk = *reinterpret_cast<const float4*>(&Qs[ck * ST + col]), sv = *reinterpret_cast<const float4*>(&As[ck * ST + col]);
#pragma unroll
            for (int v = 1; v < 4; ++v) {
                const float4 pk = *reinterpret_cast<const float4*>(&Qs[(v * 16 + ck) * ST + col]);
                const float4 pv = *reinterpret_cast<const float4*>(&As[(v * 16 + ck) * ST + col]);
                sk.x += pk.x; sk.y += pk.y; sk.z += pk.z; sk.w += pk.w;
                sv.x += pv.x; sv.y += pv.y; sv.z += pv.z; sv.w += pv.w;
            }
            const size_t off = (rowbase + ko) * D + h * HDV + col;
            *reinterpret_cast<float4*>(dK + off) = sk;
            *reinterpret_cast<float4*>(dV + off) = sv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// dQ, query-major.  Workgroup = (16 queries, key span, head, sample); wave w takes the span's key tiles 16 (4 i + w).  Lane (qi, g) owns query
// column qi of S^T = K Q^T and dP^T = V dA^T (as k_attn_dq); its query's Q, dA, LSE and Delta stay in registers.  Per key tile: P^T, the
// forward's dropout decisions (both keys of a pair in one lane), dS^T = P^T (dP^T m2 - Delta) c, then dQ^T += K^T dS^T with
// A[i][k = g] = K[key 4 g + r][NT i + j] and B = dS^T from the registers.  The 4 wave partials are added in LDS in wave order and written to
// slab `span index`: spans of 256 keys give the attn_bwd_dq_slabs(L) partial slabs, one span of every key the complete dQ in slab 0.
// ---------------------------------------------------------------------------------------------------------
template <int HDV, bool PAIR>
__global__ __launch_bounds__(256) void k_attn_wide_dq(const float* __restrict__ Q, const float* __restrict__ K,
                                                      const float* __restrict__ V, const float* __restrict__ att,
                                                      const float* __restrict__ dr, const float* __restrict__ lse,
                                                      const float* __restrict__ mask, float* __restrict__ dQ, int L, int H,
                                                      int b_off, int span, size_t slab, Drop d2, Drop d3) {
    using C = AttnWide<HDV>;
    constexpr int NC = C::NC, NT = C::NT, N4 = C::N4, ST = C::ST;
    __shared__ __attribute__((aligned(16))) float Xs[4 * 16 * ST];    // [wave][query][dim] partial dQ of each wave
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int bx, h, b;
    xcd_swizzle(bx, h, b);                         // grid (ceil(L / 16) x spans, H, B)
    const int nq = (L + 15) / 16, qb = bx % nq, sp = bx / nq;
    const size_t rowbase = (size_t)b * L;
    const int qi = lane & 15, g = lane >> 4;
    const int q = qb * 16 + qi;
    const int Lp = (L + 15) & ~15;
    const int klo = sp * span, khi = min(klo + span, Lp);
    const float scale = C::scale;
    float qa[NC], aa[NC];                          // B operands of S^T and dP^T: Q[q][g NC + c], dA[q][g NC + c]
    zero_nc<NC>(qa); zero_nc<NC>(aa);
    float dl = 0.f, lq = 0.f;
    if (q < L) {
        const size_t off = (rowbase + q) * D + h * HDV + g * NC;
        float oa[NC];
        load_nc<NC>(Q + off, qa);
        load_nc<NC>(dr + off, aa);
        load_nc<NC>(att + off, oa);
        if (d3.thresh) {
#pragma unroll
            for (int c = 0; c < NC; ++c) aa[c] *= drop_keep_scale(d3, (uint32_t)(off + c));
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) dl = fmaf(aa[c], oa[c], dl);
        lq = lse[((size_t)b * H + h) * L + q];
    }
    dl += __shfl_xor(dl, 16);
    dl += __shfl_xor(dl, 32);
    const uint32_t qrow = (uint32_t)(((size_t)(b + b_off) * H + h) * L + q);
    f32x4 dq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = klo + 16 * w; kt < khi; kt += 64) {
        float ka[NC], va[NC];                      // A operands: K[kt + qi][g NC + c], V[kt + qi][g NC + c]
        zero_nc<NC>(ka); zero_nc<NC>(va);
        if (kt + qi < L) {
            load_nc<NC>(K + (rowbase + kt + qi) * D + h * HDV + g * NC, ka);
            load_nc<NC>(V + (rowbase + kt + qi) * D + h * HDV + g * NC, va);
        }
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[c], qa[c], sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c], aa[c], dp, 0, 0, 0);
        }
        const int k4 = kt + 4 * g;                 // register r: key k4 + r, query qi
        float m2[4];
        attn_drop_q4<PAIR>(d2, qrow, L, k4, m2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __expf(sc[r] * scale + attn_key_bias(mask, rowbase, 0, k4 + r, L) - lq);
            const float ds = p * (dp[r] * m2[r] - dl) * scale;
            float kd[NT];                          // A operand: K[k4 + r][NT qi + j]
            zero_nc<NT>(kd);
            if (k4 + r < L) load_nc<NT>(K + (rowbase + k4 + r) * D + h * HDV + NT * qi, kd);
#pragma unroll
            for (int j = 0; j < NT; ++j) dq[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kd[j], ds, dq[j], 0, 0, 0);
        }
    }
    aw_park<NT>(dq, Xs + (w * 16 + qi) * ST, g);   // lane (qi, g) holds dQ^T[NT (4 g + r) + j][qi]
    __syncthreads();
    const int cq = tid >> 4, cc = tid & 15, qo = qb * 16 + cq;
    if (qo < L) {
#pragma unroll
        for (int f = 0; f < N4; ++f) {
            const int col = NT * cc + 4 * f;
            float4 a = *reinterpret_cast<const float4*>(&Xs[cq * ST + col]);
#pragma unroll
            for (int v = 1; v < 4; ++v) {
                const float4 p = *reinterpret_cast<const float4*>(&Xs[(v * 16 + cq) * ST + col]);
                a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
            }
            *reinterpret_cast<float4*>(dQ + (size_t)sp * slab + (rowbase + qo) * D + h * HDV + col) = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
void launch_attn_wide_fwd(const AttnArgs& a, hipStream_t s) {
    attn_for_head_size<128, 64>(a.H, [&](auto hd) { attn_for_bool(attn_pair_hash(a.L), [&](auto pair) {
        VSL_LAUNCH((k_attn_wide_fwd<decltype(hd)::value, decltype(pair)::value>), dim3((a.L + 15) / 16, a.H, a.B), dim3(256), 0, s, a.Q, a.K, a.V, a.mask,
                   a.att, a.lse, a.L, a.H, a.b_off, a.d2);
    }); });
}
void launch_attn_wide_bwd(const AttnArgs& a, bool query_major, hipStream_t s) {
    attn_for_head_size<128, 64>(a.H, [&](auto hd) { attn_for_bool(attn_pair_hash(a.L), [&](auto pair) {
        constexpr int HDV = decltype(hd)::value;
        constexpr bool PAIR = decltype(pair)::value;
        dynamic_lds_optin<k_attn_wide_dkv<HDV, PAIR>>(attn_wide_dkv_lds<HDV>(), "k_attn_wide_dkv");
        VSL_LAUNCH((k_attn_wide_dkv<HDV, PAIR>), dim3((a.L + 15) / 16, a.H, a.B), dim3(256), attn_wide_dkv_lds<HDV>(), s, a.Q, a.K, a.V, a.att, a.dr, a.lse,
                   a.mask, a.dK, a.dV, a.L, a.H, a.b_off, a.d2, a.d3);
        const int Lp = (a.L + 15) & ~15;
        const int spans = query_major ? 1 : attn_bwd_dq_slabs(a.L), span = query_major ? Lp : 256;
        VSL_LAUNCH((k_attn_wide_dq<HDV, PAIR>), dim3((a.L + 15) / 16 * spans, a.H, a.B), dim3(256), 0, s, a.Q, a.K, a.V, a.att, a.dr, a.lse, a.mask, a.dQ,
                   a.L, a.H, a.b_off, span, (size_t)a.B * a.L * D, a.d2, a.d3);
    }); });
}

}  // namespace vsl
