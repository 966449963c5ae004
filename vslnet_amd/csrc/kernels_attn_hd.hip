// Attention core of num_heads 4 and 16 (head sizes 32 and 8), forward and backward.  The 16-wide kernels of 8 heads: kernels_attn_h16.hip and
// k_attn_block_fwd; kernels_attn.hip routes every H = 4 / 16 shape here, L <= 128 included
// (num_heads 1 / 2, head sizes 128 / 64: kernels_attn_wide.hip).
//   a8 (:174-182)  S = Q K^T / sqrt(hd) + (1 - mask[key]) * -1e30 ; P = softmax ; O = drop(P) V
// Same contracts as the 16-wide pair: Q / K / V / att are (R, 128) rows with head h at columns h hd .. h hd + hd - 1, LSE is saved per
// (b, h, q) in natural-log units, and dQ leaves the backward as attn_bwd_dq_slabs(L) partial slabs (one per 256-key block) that k_qkv_bwd adds.
// The probability dropout is keyed exactly as the 8-head kernels key it: one drop_hash per element for L <= 256, key pairs (drop_hash_odd,
// ceil(L / 2) hashes per row) above.
// Both contractions over the head dims (S = Q K^T, dP = dA V^T) and every other product run on the fp32-input MFMA (v_mfma_f32_16x16x4_f32):
// exact fp32 products, no split planes.
#include "attn.hpp"

namespace vsl {

template <int HDV> struct AttnHd : AttnHead<HDV> {
    static_assert(HDV == 8 || HDV == 32, "head sizes 8 and 32 (16 has its own kernels)");
    static constexpr int FKB = HDV == 32 ? 128 : 256;   // forward: keys staged per block (37 KB / 25 KB of LDS)
};

// ---------------------------------------------------------------------------------------------------------
// forward.  Workgroup = (64 queries, head, sample), wave = 16 queries; lane (qi, g) owns query column qi of the transposed score tiles
// S^T = K Q^T (keys 16 t + 4 g + r), so the online softmax is lane-local up to two cross-group exchanges, in the log2 domain as in k_attn_fwd.
// K / V head slices are staged in LDS per block of FKB keys; the next block's rows travel in registers while the current one is worked on.
// ---------------------------------------------------------------------------------------------------------
template <int HDV, bool PAIR>
__global__ __launch_bounds__(256) void k_attn_hd_fwd(const float* __restrict__ Q, const float* __restrict__ K,
                                                     const float* __restrict__ V, const float* __restrict__ mask,
                                                     float* __restrict__ att, float* __restrict__ lse, int L, int H,
                                                     int b_off, Drop d2) {
    using C = AttnHd<HDV>;
    constexpr int KB = C::FKB, KST = C::KST, NC = C::NC, NT = C::NT, F4 = C::F4;
    constexpr int NJ = KB * F4 / 256;              // float4 per thread and tensor of a staged block
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;                 // [KB][KST]
    float* Vs = Ks + KB * KST;        // [KB][KST]
    float* Mb = Vs + KB * KST;        // [KB] additive key bias, log2 domain
    const int Lp = (L + 63) & ~63;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int bxs, h, b;
    xcd_swizzle(bxs, h, b);
    const size_t rowbase = (size_t)b * L;
    const int qi = lane & 15, g = lane >> 4;
    const int q = bxs * 64 + w * 16 + qi;
    const bool qok = q < L;
    float qr[NC];                                  // B operand of the S^T tiles: Q[q][g NC + c]
#pragma unroll
    for (int c = 0; c < NC; ++c) qr[c] = 0.f;
    if (qok) load_nc<NC>(Q + (rowbase + q) * D + h * HDV + g * NC, qr);
    const float c2 = C::scale * ATTN_LOG2E;      // 1 / sqrt(hd) AFTER QK^T (:175), times log2(e)
    float m = -3.0e38f, l = 0.f;
    f32x4 o[NT][2];
#pragma unroll
    for (int j = 0; j < NT; ++j) o[j][0] = o[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t qrow = (uint32_t)(((size_t)(b + b_off) * H + h) * L + q);
    const uint32_t prow = attn_drop_pair_row(qrow, L);
    const bool dropon = d2.thresh != 0u;
    float4 pk[NJ], pv[NJ];
    float pm = 0.f;
    auto fetch = [&](int kb0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int e = tid + 256 * j, key = kb0 + e / F4, c4 = (e % F4) * 4;
            pk[j] = make_float4(0.f, 0.f, 0.f, 0.f); pv[j] = pk[j];
            if (key < L) {
                pk[j] = *reinterpret_cast<const float4*>(K + (rowbase + key) * D + h * HDV + c4);
                pv[j] = *reinterpret_cast<const float4*>(V + (rowbase + key) * D + h * HDV + c4);
            }
        }
        pm = attn_key_bias(mask, rowbase, kb0, tid, L);
    };
    fetch(0);
    for (int kb0 = 0; kb0 < Lp; kb0 += KB) {
        const int nk = min(KB, Lp - kb0);          // a multiple of 64
        if (kb0) __syncthreads();                  // every wave is done with the previous block
#pragma unroll
        for (int j = 0; j < NJ; ++j) {             // (rows past L are zero)
            const int e = tid + 256 * j, kl = e / F4, c4 = (e % F4) * 4;
            *reinterpret_cast<float4*>(&Ks[kl * KST + c4]) = pk[j];
            *reinterpret_cast<float4*>(&Vs[kl * KST + c4]) = pv[j];
        }
        if (tid < KB) Mb[tid] = pm * ATTN_LOG2E;
        __syncthreads();
        if (kb0 + KB < Lp) fetch(kb0 + KB);
        for (int kt = 0; kt < nk; kt += 64) {
            // four S^T tiles: A[i = key][k = g] = K[key][g NC + c], B[k = g][j = query] = Q[q][g NC + c]
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float kr[NC];
                load_nc<NC>(&Ks[(kt + 16 * t + qi) * KST + g * NC], kr);
                s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c], qr[c], s[t], 0, 0, 0);
            }
            float x[4][4];
            float tmax = -3.0e38f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 mb = *reinterpret_cast<const float4*>(&Mb[kt + 16 * t + 4 * g]);
                x[t][0] = fmaf(s[t][0], c2, mb.x); x[t][1] = fmaf(s[t][1], c2, mb.y);
                x[t][2] = fmaf(s[t][2], c2, mb.z); x[t][3] = fmaf(s[t][3], c2, mb.w);
                tmax = fmaxf(fmaxf(tmax, fmaxf(x[t][0], x[t][1])), fmaxf(x[t][2], x[t][3]));
            }
            tmax = lane_pair16(tmax, [](float a, float bb) { return fmaxf(a, bb); });
            tmax = lane_pair32(tmax, [](float a, float bb) { return fmaxf(a, bb); });
            const float mn = fmaxf(m, tmax);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= alpha;
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[j][0][r] *= alpha; o[j][1][r] *= alpha; }
            // O^T += V^T P^T : A[i = dd][k = key] = V[key][16 j + dd], B[k = key][j = q] = P (in registers)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k4 = kb0 + kt + 16 * t + 4 * g;           // the lane's four keys k4 .. k4 + 3 (k4 even: two whole pairs)
                float pr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { pr[r] = __builtin_amdgcn_exp2f(x[t][r] - mn); l += pr[r]; }
                if constexpr (!PAIR) {
                    if (dropon) {
                        const uint32_t ei = attn_drop_elem(qrow, L, k4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) pr[r] = drop_hash(ei + r, d2.seed, d2.key) >= d2.thresh ? pr[r] * d2.scale : 0.f;
                    }
                } else if (dropon) {
                    attn_drop_pair4(d2, prow, k4, pr);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vrow = &Vs[(kt + 16 * t + 4 * g + r) * KST];
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const float vv = (HDV >= 16 || qi < HDV) ? vrow[16 * j + (qi & (HDV - 1))] : 0.f;
                        o[j][r & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, pr[r], o[j][r & 1], 0, 0, 0);
                    }
                }
            }
        }
    }
    l = lane_pair16(l, [](float a, float bb) { return a + bb; });
    l = lane_pair32(l, [](float a, float bb) { return a + bb; });
    if (qok) {
        const float inv = 1.0f / l;
        // lane (qi, g) holds O[q][dd = 16 j + 4 g + reg]
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (HDV >= 16 || g < HDV / 4)
                *reinterpret_cast<float4*>(att + (rowbase + q) * D + h * HDV + 16 * j + 4 * g) =
                    make_float4((o[j][0][0] + o[j][1][0]) * inv, (o[j][0][1] + o[j][1][1]) * inv,
                                (o[j][0][2] + o[j][1][2]) * inv, (o[j][0][3] + o[j][1][3]) * inv);
        if (g == 0 && lse) lse[((size_t)b * H + h) * L + q] = m * ATTN_LN2 + __logf(l);
    }
}

template <int HDV> constexpr size_t attn_hd_fwd_lds() { return (size_t)(2 * AttnHd<HDV>::FKB * AttnHd<HDV>::KST + AttnHd<HDV>::FKB) * sizeof(float); }

void launch_attn_hd_fwd(const AttnArgs& a, hipStream_t s) {
    attn_for_head_size<32, 8>(a.H, [&](auto hd) { attn_for_bool(attn_pair_hash(a.L), [&](auto pair) {
        constexpr int HDV = decltype(hd)::value;
        dynamic_lds_optin<k_attn_hd_fwd<HDV, decltype(pair)::value>>(attn_hd_fwd_lds<HDV>(), "k_attn_hd_fwd");
        VSL_LAUNCH((k_attn_hd_fwd<HDV, decltype(pair)::value>), dim3((a.L + 63) / 64, a.H, a.B), dim3(256), attn_hd_fwd_lds<HDV>(), s, a.Q, a.K, a.V, a.mask,
                   a.att, a.lse, a.L, a.H, a.b_off, a.d2);
    }); });
}

// ---------------------------------------------------------------------------------------------------------
// backward, single pass for every L (the scheme of k_attn_bwd_long).  Workgroup (16 waves) = (key block of 256 keys, head, sample); wave w owns
// the 16 keys of strip w, its K / V head slices in registers, K also in LDS.  The queries stream through in passes of 64 (Q, dA = dr * m3, LSE,
// D = dA . O staged per pass, the next pass' rows fetched a pass ahead):
//   phase 1: S, P, dP, dS once per (query tile, key strip); dK / dV accumulate in registers over the whole sequence; dS goes to LDS [query][key];
//   phase 2: dQ^T[dd][q] += K[key][dd] dS[q][key] over the block's keys (wave = query tile x key residue, partials added in residue order).
// dQ is a partial over this key block and goes to slab kb (slab stride = the (R, 128) tensor): as many slabs as attn_bwd_dq_slabs(L).
// Fixed summation order everywhere, no atomics.
// ---------------------------------------------------------------------------------------------------------
constexpr int AHB_KB = 256, AHB_QP = 64, AHB_DSP = AHB_KB + 4;
template <int HDV> constexpr size_t attn_hd_bwd_lds() {
    return (size_t)(AHB_KB * AttnHd<HDV>::KST + AHB_KB + AHB_QP * AHB_DSP + 2 * AHB_QP * AttnHd<HDV>::KST + 2 * AHB_QP) * sizeof(float);
}
// DQ = false (L > ATTN_SLAB_MAX_L): phase 1 alone -- dK / dV, no dS image, no dQ partials (k_attn_dq computes dQ query-major)
template <int HDV, bool PAIR, bool DQ = true>
__global__ __launch_bounds__(1024) void k_attn_hd_bwd(const float* __restrict__ Q, const float* __restrict__ K,
                                                      const float* __restrict__ V, const float* __restrict__ att,
                                                      const float* __restrict__ dr, const float* __restrict__ lse,
                                                      const float* __restrict__ mask, float* __restrict__ dQ,
                                                      float* __restrict__ dK, float* __restrict__ dV, int L, int H,
                                                      int b_off, size_t slab, Drop d2, Drop d3) {
    using C = AttnHd<HDV>;
    constexpr int KST = C::KST, NC = C::NC, NT = C::NT, F4 = C::F4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;                           // [256][KST]
    float* Mb = Ks + AHB_KB * KST;              // [256] additive key bias of the block
    float* dSs = Mb + AHB_KB;                   // [64][260] dS[query - qb][key - k0] of the current pass
    float* Qs = dSs + AHB_QP * AHB_DSP;         // [64][KST] queries of the pass
    float* As = Qs + AHB_QP * KST;              // [64][KST] dA = dr * m3
    float* Ls = As + AHB_QP * KST;              // [64] LSE
    float* Ds = Ls + AHB_QP;                    // [64] D = dA . O
    const int Lp = (L + 15) & ~15;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int kb, h, b;
    xcd_swizzle(kb, h, b);                      // grid (key blocks, H, B)
    const size_t rowbase = (size_t)b * L;
    const int k0 = kb * AHB_KB, nkeys = min(AHB_KB, Lp - k0);      // padded keys of this block (multiple of 16)
    for (int e = tid; e < AHB_KB * F4; e += 1024) {                  // the block's K slice (rows past L are zero)
        const int row = e / F4, c4 = (e % F4) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + row < L) kv = *reinterpret_cast<const float4*>(K + (rowbase + k0 + row) * D + h * HDV + c4);
        *reinterpret_cast<float4*>(&Ks[row * KST + c4]) = kv;
    }
    if (tid < AHB_KB) Mb[tid] = attn_key_bias(mask, rowbase, k0, tid, L);
    const int ki = lane & 15, g = lane >> 4;
    const float scale = C::scale;
    f32x4 dk[NT], dv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int keyl = 16 * w + ki;               // key inside the block
    const bool has_keys = 16 * w < nkeys;
    const uint32_t hb = (uint32_t)(((size_t)(b + b_off) * H + h) * L);
    // B operands of the strip's tiles (column = key ki, k group g): K[key][g NC + c] and V[key][g NC + c]
    float kr[NC], vr[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) kr[c] = vr[c] = 0.f;
    if (has_keys && k0 + keyl < L) {
        load_nc<NC>(K + (rowbase + k0 + keyl) * D + h * HDV + g * NC, kr);
        load_nc<NC>(V + (rowbase + k0 + keyl) * D + h * HDV + g * NC, vr);
    }
    // rows of the next pass, requested a pass ahead: threads 0 .. 16 HDV - 1 own one float4 of Q, dA and att each
    constexpr int NSTG = AHB_QP * F4;
    float4 nq, na, no;
    float nl = 0.f;
    auto fetch = [&](int qb) {
        const int row = qb + tid / F4, c4 = (tid % F4) * 4;
        nq = make_float4(0.f, 0.f, 0.f, 0.f); na = nq; no = nq; nl = 0.f;
        if (tid < NSTG && row < L) {
            const size_t off = (rowbase + row) * D + h * HDV + c4;
            nq = *reinterpret_cast<const float4*>(Q + off);
            na = *reinterpret_cast<const float4*>(dr + off);
            no = *reinterpret_cast<const float4*>(att + off);
            if (tid % F4 == 0) nl = lse[((size_t)b * H + h) * L + row];
        }
    };
    auto stage = [&](int qb) {                  // (the previous pass' readers are behind a barrier; NSTG is a multiple of 64: whole waves)
        if (tid < NSTG) {
            const int rl = tid / F4, c4 = (tid % F4) * 4;
            float4 av = na;
            if (d3.thresh && qb + rl < L) {     // r = drop3(att) + x  (:183-184)
                const uint32_t base = (uint32_t)((rowbase + qb + rl) * D + h * HDV + c4);
                av.x *= drop_mul(d3, base); av.y *= drop_mul(d3, base + 1);
                av.z *= drop_mul(d3, base + 2); av.w *= drop_mul(d3, base + 3);
            }
            *reinterpret_cast<float4*>(&Qs[rl * KST + c4]) = nq;
            *reinterpret_cast<float4*>(&As[rl * KST + c4]) = av;
            float dsum = av.x * no.x + av.y * no.y + av.z * no.z + av.w * no.w;     // D_q = dA . O (= sum_k dP_k P_k)
#pragma unroll
            for (int sh = 1; sh < F4; sh <<= 1) dsum += __shfl_xor(dsum, sh);
            if (tid % F4 == 0) { Ds[rl] = dsum; Ls[rl] = nl; }
        }
    };
    fetch(0);
    __syncthreads();
    const float mbk = Mb[keyl];
    for (int qb = 0; qb < Lp; qb += AHB_QP) {
        const int qe = min(qb + AHB_QP, Lp);
        stage(qb);
        if (qb + AHB_QP < Lp) fetch(qb + AHB_QP);
        __syncthreads();
        if (has_keys) {
            for (int qt = qb; qt < qe; qt += 16) {
                const int ql0 = qt - qb;
                // S = Q K^T and dP = dA V^T: A[i = query][k = g] = Q[q][g NC + c] (resp. dA), B[k = g][j = key] = K[key][g NC + c] (resp. V)
                float qa[NC], aa[NC];
                load_nc<NC>(&Qs[(ql0 + ki) * KST + g * NC], qa);
                load_nc<NC>(&As[(ql0 + ki) * KST + g * NC], aa);
                f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[c], kr[c], sc, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[c], vr[c], dp, 0, 0, 0);
                }
                float m2v[4] = {1.f, 1.f, 1.f, 1.f};    // dropout of the probabilities as the forward drew it
                if (!PAIR) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) m2v[r] = drop_mul(d2, attn_drop_elem(hb + (uint32_t)(qb + ql0 + 4 * g + r), L, k0 + keyl));
                } else if (d2.thresh != 0u) {
                    const uint32_t Lh = attn_drop_pair_stride(L), kp = (uint32_t)((k0 + keyl) >> 1);
                    const int odd = ki & 1;
                    uint32_t hm[2], hp[2];
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        hm[jj] = drop_hash((hb + (uint32_t)(qb + ql0 + 4 * g + 2 * odd + jj)) * Lh + kp, d2.seed, d2.key);
                        hp[jj] = __float_as_uint(lane_xor1(__uint_as_float(hm[jj])));
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) m2v[r] = attn_drop_pair_mul(d2, odd, (r >> 1) == odd ? hm[r & 1] : hp[r & 1]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = ql0 + 4 * g + r;
                    const float p = __expf(sc[r] * scale + mbk - Ls[ql]);
                    const float m2 = m2v[r];
                    const float pd = p * m2;
                    const float ds = p * (dp[r] * m2 - Ds[ql]) * scale;
                    if (DQ) dSs[ql * AHB_DSP + keyl] = ds;
                    // dV^T[dd][key] += dA[q][dd] P[q][key] ; dK^T[dd][key] += Q[q][dd] dS[q][key]   (A[i = dd][k = query])
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const bool in = HDV >= 16 || ki < HDV;
                        const float a_dd = in ? As[ql * KST + 16 * j + (ki & (HDV - 1))] : 0.f;
                        const float q_dd = in ? Qs[ql * KST + 16 * j + (ki & (HDV - 1))] : 0.f;
                        dv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_dd, pd, dv[j], 0, 0, 0);
                        dk[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(q_dd, ds, dk[j], 0, 0, 0);
                    }
                }
            }
        }
        if constexpr (DQ) {
        __syncthreads();                        // dS of this pass complete
        const int qt2 = qb + 16 * (w & 3), kres = w >> 2;
        f32x4 dqs[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) dqs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (qt2 < qe) {
            f32x4 dq[NT][4];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) dq[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* sp = dSs + (16 * (w & 3) + ki) * AHB_DSP + g;
            const bool in = HDV >= 16 || ki < HDV;
            for (int kk = 16 * kres; kk < nkeys; kk += 64) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kk + 4 * i + g;
                    const float sb = sp[kk + 4 * i];
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const float ka = in ? Ks[key * KST + 16 * j + (ki & (HDV - 1))] : 0.f;
                        dq[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, sb, dq[j][i], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) dqs[j][c] = (dq[j][0][c] + dq[j][1][c]) + (dq[j][2][c] + dq[j][3][c]);
        }
        __syncthreads();                        // every wave has read its dS rows: the buffer becomes the exchange area
        float4* xq = reinterpret_cast<float4*>(dSs);          // [3 residues][4 query tiles][NT][64 lanes]
        if (kres > 0)
#pragma unroll
            for (int j = 0; j < NT; ++j) xq[(((kres - 1) * 4 + (w & 3)) * NT + j) * 64 + lane] = make_float4(dqs[j][0], dqs[j][1], dqs[j][2], dqs[j][3]);
        __syncthreads();
        if (kres == 0 && qt2 < qe) {
            const int q = qt2 + ki;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float4 p1 = xq[((0 * 4 + w) * NT + j) * 64 + lane], p2 = xq[((1 * 4 + w) * NT + j) * 64 + lane],
                             p3 = xq[((2 * 4 + w) * NT + j) * 64 + lane];
                if (q < L && (HDV >= 16 || g < HDV / 4))
                    *reinterpret_cast<float4*>(dQ + (size_t)kb * slab + (rowbase + q) * D + h * HDV + 16 * j + 4 * g) =
                        make_float4(((dqs[j][0] + p1.x) + p2.x) + p3.x, ((dqs[j][1] + p1.y) + p2.y) + p3.y,
                                    ((dqs[j][2] + p1.z) + p2.z) + p3.z, ((dqs[j][3] + p1.w) + p2.w) + p3.w);
            }
        }
        }
        __syncthreads();                        // dS buffer, Qs / As / Ls / Ds free for the next pass
    }
    if (has_keys && k0 + keyl < L) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (HDV >= 16 || g < HDV / 4) {
                const size_t off = (rowbase + k0 + keyl) * D + h * HDV + 16 * j + 4 * g;
                *reinterpret_cast<float4*>(dK + off) = make_float4(dk[j][0], dk[j][1], dk[j][2], dk[j][3]);
                *reinterpret_cast<float4*>(dV + off) = make_float4(dv[j][0], dv[j][1], dv[j][2], dv[j][3]);
            }
    }
}

template <int HDV, bool PAIR, bool DQ> static void attn_hd_bwd_go(const AttnArgs& a, hipStream_t s) {
    const int Lp = (a.L + 15) & ~15;
    dynamic_lds_optin<k_attn_hd_bwd<HDV, PAIR, DQ>>(attn_hd_bwd_lds<HDV>(), "k_attn_hd_bwd");
    VSL_LAUNCH((k_attn_hd_bwd<HDV, PAIR, DQ>), dim3((Lp + AHB_KB - 1) / AHB_KB, a.H, a.B), dim3(1024), attn_hd_bwd_lds<HDV>(), s, a.Q, a.K, a.V, a.att, a.dr,
               a.lse, a.mask, a.dQ, a.dK, a.dV, a.L, a.H, a.b_off, (size_t)a.B * a.L * D, a.d2, a.d3);
}
void launch_attn_hd_bwd(const AttnArgs& a, bool dq, hipStream_t s) {
    attn_for_head_size<32, 8>(a.H, [&](auto hd) {
        constexpr int HDV = decltype(hd)::value;
        if (!dq) attn_hd_bwd_go<HDV, true, false>(a, s);       // L > ATTN_SLAB_MAX_L (key pairs): dK / dV per key block, dQ from k_attn_dq
        else attn_for_bool(attn_pair_hash(a.L), [&](auto pair) { attn_hd_bwd_go<HDV, decltype(pair)::value, true>(a, s); });
    });
}

}  // namespace vsl
