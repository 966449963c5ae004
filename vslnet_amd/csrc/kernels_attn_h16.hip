// Attention core of num_heads 8 (head size 16), sequences of L > 128 forward and every L backward (L <= 128 forward: k_attn_block_fwd,
// kernels_enc.hip).  S = Q K^T and dP = dA V^T run on the bf16 matrix cores at fp32 grade (three split planes), every other product on the
// fp32-input MFMA.  The other head counts: kernels_attn_hd.hip (4 / 16), kernels_attn_wide.hip (1 / 2); query-major dQ: kernels_attn.hip.
#include "attn.hpp"
#include "stamps.hpp"

namespace vsl {

// =========================================================================================================
// a8 (attention core)  S = Q K^T / sqrt(hd) + (1 - mask[key]) * -1e30 ; P = softmax ; O = drop(P) V   (:174-182), sequences of L > 256
//   head size 16, fp32 MFMA 16x16x4.  Workgroup = (64 queries, head, sample); wave = 16 queries.
//   K/V head slices live in LDS; scores are computed transposed (S^T = K Q^T) so every lane owns one query column:
//   online softmax is lane-local (+2 shuffles across the 4 key groups) and P feeds the PV MFMA from registers.
//   Saves LSE = m + log(l) per (b, h, q) for the backward.
// Round 6: the key loop was issue-bound (765 cycles per 16-key tile and wave, 256 of them matrix work): it now takes 64 keys per turn -- four
// independent S tiles, ONE running-maximum update (2 shuffles, 1 rescale) per 64 keys instead of per 16 --, works in the log2 domain (x = S c +
// bias with c = log2(e) / 4: v_exp_f32 directly, LSE converted back at the end), draws two dropout decisions from every hash (drop_hash_odd) and
// feeds PV into two alternating accumulators.
// =========================================================================================================
#ifndef VSL_AF_KB
#define VSL_AF_KB 256
#endif
constexpr int AF_KB = VSL_AF_KB;    // keys staged per block: 45 KB of LDS whatever L is -> 3 workgroups per CU at L = 1024
constexpr int AF_NJ = AF_KB * 4 / 256;
// PAIR: two dropout decisions per hash (L > 256) ; false: one hash per element, the masks of L <= 256 (the kernel then serves 128 < L <= 256 too)
template <bool PAIR>
__global__ __launch_bounds__(256) void k_attn_fwd(const float* __restrict__ Q, const float* __restrict__ K,
                                                  const float* __restrict__ V, const float* __restrict__ mask,
                                                  float* __restrict__ att, float* __restrict__ lse, int L, int H,
                                                  int b_off, Drop d2) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Lp = (L + 63) & ~63;                 // keys in turns of 64 (the pad keys carry the mask bias and zero K / V)
    const int KB = min(Lp, AF_KB);
    constexpr int kst = 20;
    float* Vs = smem;                 // [KB][20]  V head slice of the current key block
    float* Mb = Vs + KB * kst;        // [KB] additive key bias, log2 domain
    uint16_t* Kp = reinterpret_cast<uint16_t*>(Mb + KB);      // [3 terms][KB][16] bf16: the K head slice, split once per block (af_kp)
    const int KPL = KB * 16;          // elements per plane
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int bxs, h, b;
    xcd_swizzle(bxs, h, b);                        // all heads of a sample on one XCD: its rows are fetched into one L2
    const size_t rowbase = (size_t)b * L;
    const int qi = lane & 15, g = lane >> 4;
    const int q = bxs * 64 + w * 16 + qi;
    const bool qok = q < L;
    // S^T = K Q^T on the bf16 matrix cores at fp32 grade: v_mfma_f32_16x16x32_bf16 contracts over 32 = TWO products of the 16 head dims, so
    // the six products of the 3-way split are three instructions (they overlap with the vector work of the SIMD's other waves; the fp32-input
    // MFMA does not: tools/ubench/split_bf16.hip):  [kh | km] x [qh | qh] + [kh | kl] x [qm | qh] + [kh | km] x [ql | qm].
    // lane (i, g): k group g < 2 = dims 8 g .. of the first term, g >= 2 = dims 8 (g - 2) .. of the second.
    u32x4_t bq1, bq2, bq3;
    {
        float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qb = qa;
        if (qok) {
            const float* qp = Q + (rowbase + q) * D + h * HD + 8 * (g & 1);
            qa = *reinterpret_cast<const float4*>(qp);
            qb = *reinterpret_cast<const float4*>(qp + 4);
        }
        uint32_t th[4], tm[4], tl[4];
        split3(qa.x, qa.y, th[0], tm[0], tl[0]); split3(qa.z, qa.w, th[1], tm[1], tl[1]);
        split3(qb.x, qb.y, th[2], tm[2], tl[2]); split3(qb.z, qb.w, th[3], tm[3], tl[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bq1[e] = th[e]; bq2[e] = g < 2 ? tm[e] : th[e]; bq3[e] = g < 2 ? tl[e] : tm[e]; }
    }
    // A operands of a key tile: planes (h | m) and (h | l) by k group
    const int ka1 = (g < 2 ? 0 : 1) * KPL + af_kp(qi, g & 1), ka2 = (g < 2 ? 0 : 2) * KPL + af_kp(qi, g & 1);
    const float c2 = AttnHead<HD>::scale * ATTN_LOG2E;             // 1 / sqrt(16), applied AFTER QK^T like the reference (:175), times log2(e)
    float m = -3.0e38f, l = 0.f;
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    const uint32_t prow = (uint32_t)(((size_t)(b + b_off) * H + h) * L + q) * attn_drop_pair_stride(L);     // = attn_drop_pair_row(qrow, L): dropout of the probabilities, attn.hpp
    const bool dropon = d2.thresh != 0u;
    // the rows of the NEXT key block travel in registers while the current one is worked on (8 float4 per thread): a block's global-memory
    // latency used to be exposed at every block boundary -- a third of the kernel's time with three workgroups per CU to hide it
    float4 pk[AF_NJ], pv[AF_NJ];
    float pm = 0.f;
    auto fetch = [&](int kb0) {
        const int nk = min(AF_KB, Lp - kb0);
#pragma unroll
        for (int j = 0; j < AF_NJ; ++j) {
            const int e = tid + 256 * j, key = kb0 + (e >> 2), c4 = (e & 3) * 4;
            pk[j] = make_float4(0.f, 0.f, 0.f, 0.f); pv[j] = pk[j];
            if (e < nk * 4 && key < L) {
                pk[j] = *reinterpret_cast<const float4*>(K + (rowbase + key) * D + h * HD + c4);
                pv[j] = *reinterpret_cast<const float4*>(V + (rowbase + key) * D + h * HD + c4);
            }
        }
        pm = attn_key_bias(mask, rowbase, kb0, tid, L);
    };
    fetch(0);
    for (int kb0 = 0; kb0 < Lp; kb0 += AF_KB) {
        const int nk = min(AF_KB, Lp - kb0);
        if (kb0) __syncthreads();                  // every wave is done with the previous block
#pragma unroll
        for (int j = 0; j < AF_NJ; ++j) {
            const int e = tid + 256 * j, kl = e >> 2, c4 = (e & 3) * 4;
            if (e < nk * 4) {
                uint32_t h0, m0, l0, h1, m1, l1;
                split3(pk[j].x, pk[j].y, h0, m0, l0);
                split3(pk[j].z, pk[j].w, h1, m1, l1);
                uint16_t* kd = Kp + af_kp(kl, c4 >> 3) + (c4 & 7);
                *reinterpret_cast<u32x2_t*>(kd) = u32x2_t{h0, h1};
                *reinterpret_cast<u32x2_t*>(kd + KPL) = u32x2_t{m0, m1};
                *reinterpret_cast<u32x2_t*>(kd + 2 * KPL) = u32x2_t{l0, l1};
                *reinterpret_cast<float4*>(&Vs[kl * kst + c4]) = pv[j];
            }
        }
        if (tid < nk) Mb[tid] = pm * ATTN_LOG2E;
        __syncthreads();
        if (kb0 + AF_KB < Lp) fetch(kb0 + AF_KB);
        for (int kt = 0; kt < nk; kt += 64) {
            // four S^T tiles: rows = keys kb0 + kt + 16 t + 4 g + reg, col = query qi
            f32x4 s[4];
            u32x4_t a1[4], a2[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a1[t] = *reinterpret_cast<const u32x4_t*>(Kp + ka1 + (kt + 16 * t) * 16);
                a2[t] = *reinterpret_cast<const u32x4_t*>(Kp + ka2 + (kt + 16 * t) * 16);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = mfma16_bf16(a1[t], bq3, f32x4{0.f, 0.f, 0.f, 0.f});       // hl + mm (small terms first)
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = mfma16_bf16(a2[t], bq2, s[t]);                            // hm + lh
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = mfma16_bf16(a1[t], bq1, s[t]);                            // hh + mh
            float x[4][4];
            float tmax = -3.0e38f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 mb = *reinterpret_cast<const float4*>(&Mb[kt + 16 * t + 4 * g]);
                x[t][0] = fmaf(s[t][0], c2, mb.x); x[t][1] = fmaf(s[t][1], c2, mb.y);
                x[t][2] = fmaf(s[t][2], c2, mb.z); x[t][3] = fmaf(s[t][3], c2, mb.w);
                tmax = fmaxf(fmaxf(tmax, fmaxf(x[t][0], x[t][1])), fmaxf(x[t][2], x[t][3]));
            }
            tmax = lane_pair16(tmax, [](float a, float b) { return fmaxf(a, b); });
            tmax = lane_pair32(tmax, [](float a, float b) { return fmaxf(a, b); });
            const float mn = fmaxf(m, tmax);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
            // O^T += V^T P^T : A[i = dd][k = key] = V[key][dd], B[k = key][j = q] = P (in registers); fp32-input MFMA (P would have to be split per tile)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float pr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { pr[r] = __builtin_amdgcn_exp2f(x[t][r] - mn); l += pr[r]; }
                if constexpr (!PAIR) {
                    if (dropon) {
                        const uint32_t ei = attn_drop_elem((uint32_t)(((size_t)(b + b_off) * H + h) * L + q), L, kb0 + kt + 16 * t + 4 * g);
#pragma unroll
                        for (int r = 0; r < 4; ++r) pr[r] = drop_hash(ei + r, d2.seed, d2.key) >= d2.thresh ? pr[r] * d2.scale : 0.f;
                    }
                } else if (dropon) {
                    attn_drop_pair4(d2, prow, kb0 + kt + 16 * t + 4 * g, pr);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float vv = Vs[(kt + 16 * t + 4 * g + r) * kst + qi];
                    if (r & 1) o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, pr[r], o1, 0, 0, 0);
                    else o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, pr[r], o0, 0, 0, 0);
                }
            }
        }
    }
    l = lane_pair16(l, [](float a, float b) { return a + b; });
    l = lane_pair32(l, [](float a, float b) { return a + b; });
    if (qok) {
        const float inv = 1.0f / l;
        // lane (qi, g) holds O[q][dd = 4g + reg]
        *reinterpret_cast<float4*>(att + (rowbase + q) * D + h * HD + 4 * g) =
            make_float4((o0[0] + o1[0]) * inv, (o0[1] + o1[1]) * inv, (o0[2] + o1[2]) * inv, (o0[3] + o1[3]) * inv);
        if (g == 0 && lse) lse[((size_t)b * H + h) * L + q] = m * ATTN_LN2 + __logf(l);      // (null in inference mode)
    }
}
void launch_attn_h16_fwd(const AttnArgs& a, hipStream_t s) {
    const int Lp = (a.L + 63) & ~63;
    const int KB = Lp < AF_KB ? Lp : AF_KB;
    const size_t shm = (size_t)(KB * 20 + KB) * sizeof(float) + (size_t)3 * KB * 16 * sizeof(uint16_t);
    attn_for_bool(attn_pair_hash(a.L), [&](auto pair) {      // false: the kernel then serves 128 < L <= 256 too
        dynamic_lds_optin<k_attn_fwd<decltype(pair)::value>>(shm, "k_attn_fwd");
        VSL_LAUNCH(k_attn_fwd<decltype(pair)::value>, dim3((a.L + 63) / 64, a.H, a.B), dim3(256), shm, s, a.Q, a.K, a.V, a.mask, a.att, a.lse, a.L, a.H, a.b_off, a.d2);
    });
}

// Fused attention backward for Lp <= 128: ONE workgroup (16 waves) per (sample, head) computes S, P, dP and dS once.
// Queries are processed in passes of 64 so that dS[64][keys] fits beside the head slices in < 80 KB of LDS: two workgroups
// share a CU (one stages while the other computes) and a weight-gradient workgroup of another stream still fits too.
//   phase 1: wave (ks = w & 7, qh = w >> 3) owns the 16 keys of strip ks and the query tiles qh, qh + 2 of the pass;
//            dK / dV of the strip accumulate in registers over all passes, dS goes to LDS as a [query][key] matrix;
//   phase 2: waves 0-3 each multiply the 16 rows of dS of one query tile with K  ->  dQ (4 independent MFMA chains).
// The two dK / dV partials (qh = 0, 1) are added in a fixed order through LDS, so the result does not depend on
// scheduling.  Against the two-kernel path this halves the exp / dropout-hash / S / dP work (fp32 MFMAs and the vector ALU
// share the SIMD, so that work is not hidden behind anything) and removes one kernel boundary.
// LMAX = 128: 8 key strips x 2 query halves (the two dK / dV partials are added through LDS); LMAX = 256: 16 key strips, a
// wave sees every query tile (no exchange), 152 KB of LDS, one workgroup per CU.
constexpr int AB_KST = 20, AB_QP = 64;
template <int LMAX> constexpr size_t ab_lds() { return (size_t)(4 * LMAX * AB_KST + AB_QP * (LMAX + 4) + 3 * LMAX) * sizeof(float); }
template <int LMAX>
__global__ __launch_bounds__(1024) void k_attn_bwd_fused(const float* __restrict__ Q, const float* __restrict__ K,
                                                         const float* __restrict__ V, const float* __restrict__ att,
                                                         const float* __restrict__ dr, const float* __restrict__ lse,
                                                         const float* __restrict__ mask, float* __restrict__ dQ,
                                                         float* __restrict__ dK, float* __restrict__ dV, int L, int H,
                                                         int b_off, Drop d2, Drop d3) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int AB_LMAX = LMAX, AB_DSP = LMAX + 4, NKS = LMAX / 16, NSPLIT = 16 / NKS;
    float* Ks = smem;                           // [LMAX][20]
    float* dSs = Ks + AB_LMAX * AB_KST;         // [64][132]   dS[query - qb][key] of the current pass
    float* Ls = dSs + AB_QP * AB_DSP;           // LSE per query
    float* Ds = Ls + AB_LMAX;                   // D = dA . O per query
    float* Mb = Ds + AB_LMAX;                   // additive key bias
    float* Qs = Mb + AB_LMAX;                   // [128][20]   Qs | Vs | As are dead after the last pass and become the
    float* Vs = Qs + AB_LMAX * AB_KST;          // [128][20]   exchange area of the dK / dV partials
    float* As = Vs + AB_LMAX * AB_KST;          // [128][20]   dA = dr * m3
    const int Lp = (L + 15) & ~15;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int h, b, bzs;
    xcd_swizzle(h, b, bzs);                     // grid (H, B): all heads of a sample on one XCD (common.hpp)
    const size_t rowbase = (size_t)b * L;
    STAMP(0);
    for (int it = 0; it < LMAX / 128; ++it) {
        const int e = (tid & 511) + 512 * it, row = e >> 2, c4 = (e & 3) * 4;
        const size_t off = (rowbase + row) * D + h * HD + c4;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < 512) {
            float4 qv = z, kv = z;
            if (row < L) {
                qv = *reinterpret_cast<const float4*>(Q + off);
                kv = *reinterpret_cast<const float4*>(K + off);
            }
            *reinterpret_cast<float4*>(&Qs[row * AB_KST + c4]) = qv;
            *reinterpret_cast<float4*>(&Ks[row * AB_KST + c4]) = kv;
            if (it == 0 && tid < AB_LMAX) {
                Ls[tid] = tid < L ? lse[((size_t)b * H + h) * L + tid] : 0.f;
                Mb[tid] = attn_key_bias(mask, rowbase, 0, tid, L);
            }
        } else {
            float4 vv = z, av = z, ov = z;
            if (row < L) {
                vv = *reinterpret_cast<const float4*>(V + off);
                av = *reinterpret_cast<const float4*>(dr + off);
                ov = *reinterpret_cast<const float4*>(att + off);
                if (d3.thresh) {                    // r = drop3(att) + x  (:183-184)
                    const uint32_t base = (uint32_t)off;
                    av.x *= drop_mul(d3, base); av.y *= drop_mul(d3, base + 1);
                    av.z *= drop_mul(d3, base + 2); av.w *= drop_mul(d3, base + 3);
                }
            }
            *reinterpret_cast<float4*>(&Vs[row * AB_KST + c4]) = vv;
            *reinterpret_cast<float4*>(&As[row * AB_KST + c4]) = av;
            float dsum = av.x * ov.x + av.y * ov.y + av.z * ov.z + av.w * ov.w;     // D_q = dA . O (= sum_k dP_k P_k)
            dsum += lane_xor1(dsum);
            dsum += lane_xor2(dsum);
            if ((e & 3) == 0) Ds[row] = dsum;
        }
    }
    STAMP(1);
    __syncthreads();
    STAMP(2);
    const int ki = lane & 15, g = lane >> 4;
    const int hi = w / NKS;                     // which of the NSPLIT dK / dV partials this wave produces
    const float scale = AttnHead<HD>::scale;
    f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    const int key = 16 * (w % NKS) + ki;
    const bool has_keys = 16 * (w % NKS) < Lp;
    float4 kf = make_float4(0.f, 0.f, 0.f, 0.f), vf = kf;
    float mb = MASK_VALUE;
    if (has_keys) {
        kf = *reinterpret_cast<const float4*>(&Ks[key * AB_KST + 4 * g]);
        vf = *reinterpret_cast<const float4*>(&Vs[key * AB_KST + 4 * g]);
        mb = Mb[key];
    }
    const uint32_t hb = (uint32_t)(((size_t)(b + b_off) * H + h) * L);
    for (int qb = 0; qb < Lp; qb += AB_QP) {
        const int qe = min(qb + AB_QP, Lp);
        if (has_keys) {
            for (int qt = qb + 16 * hi; qt < qe; qt += 16 * NSPLIT) {
                // S tile (rows = queries qt + 4g + reg, col = key) and dPd tile, same shape
                const float4 qa = *reinterpret_cast<const float4*>(&Qs[(qt + ki) * AB_KST + 4 * g]);
                const float4 aa = *reinterpret_cast<const float4*>(&As[(qt + ki) * AB_KST + 4 * g]);
                f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.x, kf.x, sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa.x, vf.x, dp, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.y, kf.y, sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa.y, vf.y, dp, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.z, kf.z, sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa.z, vf.z, dp, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.w, kf.w, sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(aa.w, vf.w, dp, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qq = qt + 4 * g + r;
                    const float p = __expf(sc[r] * scale + mb - Ls[qq]);
                    const float m2 = drop_mul(d2, (hb + (uint32_t)qq) * (uint32_t)L + (uint32_t)key);
                    const float pd = p * m2;
                    const float ds = p * (dp[r] * m2 - Ds[qq]) * scale;
                    dSs[(qq - qb) * AB_DSP + key] = ds;
                    // dV^T[dd][key] += dA[q][dd] * Pd[q][key] ; dK^T[dd][key] += Q[q][dd] * dS[q][key]
                    dv = __builtin_amdgcn_mfma_f32_16x16x4f32(As[qq * AB_KST + ki], pd, dv, 0, 0, 0);
                    dk = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[qq * AB_KST + ki], ds, dk, 0, 0, 0);
                }
            }
        }
        if (qb == 0) STAMP(3);
        __syncthreads();                        // dS of this pass complete
        if (qb == 0) STAMP(4);
        // phase 2: dQ^T[dd][q] += K[key][dd] * dS[q][key].  All 16 waves: wave = (query tile w & 3, key-tile residue w >> 2 mod 4); the four
        // partial tiles of a query tile meet in the (then dead) dS buffer and are added in residue order.  (One query tile per wave over
        // every key kept 12 of the 16 waves idle for a third of the pass.)
        const int qt2 = qb + 16 * (w & 3), kr = w >> 2;
        f32x4 dqs = {0.f, 0.f, 0.f, 0.f};
        if (qt2 < qe) {
            f32x4 dq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* kp = Ks + g * AB_KST + ki;
            const float* sp = dSs + (16 * (w & 3) + ki) * AB_DSP + g;
            for (int k0 = 16 * kr; k0 < Lp; k0 += 64) {
                float ka[4], sb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { ka[i] = kp[(k0 + 4 * i) * AB_KST]; sb[i] = sp[k0 + 4 * i]; }
#pragma unroll
                for (int i = 0; i < 4; ++i) dq[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[i], sb[i], dq[i], 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) dqs[c] = (dq[0][c] + dq[1][c]) + (dq[2][c] + dq[3][c]);
        }
        __syncthreads();                        // every wave has read its dS rows: the buffer becomes the exchange area
        float4* xq = reinterpret_cast<float4*>(dSs);          // [3 residues][4 query tiles][64 lanes]
        if (kr > 0) xq[((kr - 1) * 4 + (w & 3)) * 64 + lane] = make_float4(dqs[0], dqs[1], dqs[2], dqs[3]);
        __syncthreads();
        if (kr == 0 && qt2 < qe) {
            const float4 p1 = xq[(0 * 4 + w) * 64 + lane], p2 = xq[(1 * 4 + w) * 64 + lane], p3 = xq[(2 * 4 + w) * 64 + lane];
            const int q = qt2 + ki;
            if (q < L)
                *reinterpret_cast<float4*>(dQ + (rowbase + q) * D + h * HD + 4 * g) =
                    make_float4(((dqs[0] + p1.x) + p2.x) + p3.x, ((dqs[1] + p1.y) + p2.y) + p3.y,
                                ((dqs[2] + p1.z) + p2.z) + p3.z, ((dqs[3] + p1.w) + p2.w) + p3.w);
        }
        if (qb == 0) STAMP(5);
        __syncthreads();                        // dS buffer (and, after the last pass, Qs / Vs / As) free
        if (qb == 0) STAMP(6);
    }
    float* xkv = Qs;                            // [8 strips][64 lanes][8]
    if (NSPLIT == 2 && hi == 1) {
        *reinterpret_cast<float4*>(&xkv[((w & 7) * 64 + lane) * 8]) = make_float4(dk[0], dk[1], dk[2], dk[3]);
        *reinterpret_cast<float4*>(&xkv[((w & 7) * 64 + lane) * 8 + 4]) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    }
    __syncthreads();
    if (hi == 0 && key < L) {
        float4 k1 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = k1;
        if (NSPLIT == 2) {
            k1 = *reinterpret_cast<const float4*>(&xkv[((w & 7) * 64 + lane) * 8]);
            v1 = *reinterpret_cast<const float4*>(&xkv[((w & 7) * 64 + lane) * 8 + 4]);
        }
        const size_t off = (rowbase + key) * D + h * HD + 4 * g;
        *reinterpret_cast<float4*>(dK + off) = make_float4(dk[0] + k1.x, dk[1] + k1.y, dk[2] + k1.z, dk[3] + k1.w);
        *reinterpret_cast<float4*>(dV + off) = make_float4(dv[0] + v1.x, dv[1] + v1.y, dv[2] + v1.z, dv[3] + v1.w);
    }
    STAMP(7);
}
// Single-pass attention backward for L > 256 (round 3; replaces k_attn_bwd_dq + k_attn_bwd_dkv, which computed S, P, dP and dS twice).
// Workgroup (16 waves) = (key block of 256 keys, head, sample).  The block's K / V head slices stay in LDS; the queries stream through in
// passes of 64 (Q, dA = dr * m3, LSE, D = dA . O staged per pass).  Per pass, as in k_attn_bwd_fused<256>:
//   phase 1: wave w owns the 16 keys of strip w and all four query tiles of the pass: S, P, dP, dS ONCE; dK / dV of the strip accumulate
//            in registers over every pass of the sequence; dS goes to LDS as a [query][key] matrix;
//   phase 2: dQ^T[dd][q] += K[key][dd] dS[q][key] over the block's keys (wave = query tile x key residue, partials added in residue order).
// dK / dV are complete; dQ is a partial over this key block and goes to slab `kb` of dQ (slab stride = the (R, 128) tensor): k_qkv_bwd adds
// the slabs while it stages its tile (and leaves the sum in slab 0 for the weight gradient).  122 KB of LDS, one workgroup per CU.
constexpr int ABL_KB = 256;
constexpr size_t abl_lds() { return (size_t)(2 * ABL_KB * AB_KST + ABL_KB + AB_QP * (ABL_KB + 4) + 2 * AB_QP * AB_KST + 2 * AB_QP) * sizeof(float) + (size_t)2 * 3 * AB_QP * 16 * sizeof(uint16_t); }
// PAIR: the probability site's masks are keyed by key PAIRS (the forward of L > 256, k_attn_fwd) ; false: one hash per element (the forward of
// L <= 256, k_attn_block_fwd) -- the kernel then serves 128 < L <= 256 as ONE key block (launch_attn_h16_bwd)
// DQ = false (L > ATTN_SLAB_MAX_L): phase 1 alone -- dK / dV, no dS image, no dQ partials (k_attn_dq computes dQ query-major)
template <bool PAIR, bool DQ = true>
__global__ __launch_bounds__(1024) void k_attn_bwd_long(const float* __restrict__ Q, const float* __restrict__ K,
                                                        const float* __restrict__ V, const float* __restrict__ att,
                                                        const float* __restrict__ dr, const float* __restrict__ lse,
                                                        const float* __restrict__ mask, float* __restrict__ dQ,
                                                        float* __restrict__ dK, float* __restrict__ dV, int L, int H,
                                                        int b_off, size_t slab, Drop d2, Drop d3) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int AB_DSP = ABL_KB + 4;
    float* Ks = smem;                           // [256][20]
    float* Vs = Ks + ABL_KB * AB_KST;           // [256][20]
    float* Mb = Vs + ABL_KB * AB_KST;           // additive key bias of the block
    float* dSs = Mb + ABL_KB;                   // [64][260] dS[query - qb][key - k0] of the current pass
    float* Qs = dSs + AB_QP * AB_DSP;           // [64][20] queries of the pass
    float* As = Qs + AB_QP * AB_KST;            // [64][20] dA = dr * m3
    float* Ls = As + AB_QP * AB_KST;            // [64] LSE
    float* Ds = Ls + AB_QP;                     // [64] D = dA . O
    // S = Q K^T and dP = dA V^T contract over the 16 head dims: on the bf16 matrix cores at fp32 grade like k_attn_fwd's K Q^T (three
    // v_mfma_f32_16x16x32_bf16 per product: the six split products, two per instruction) -- 96 pipe cycles that overlap with the vector work instead
    // of 256 of the fp32-input MFMA that do not.  Q and dA of the pass are split ONCE by the staging threads into three bf16 planes each.
    uint16_t* Qp = reinterpret_cast<uint16_t*>(Ds + AB_QP);     // [3 terms][64][16] (af_kp)
    uint16_t* Ap = Qp + 3 * AB_QP * 16;                         // [3 terms][64][16]
    constexpr int QPL = AB_QP * 16;
    const int Lp = (L + 15) & ~15;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int kb, h, b;
    xcd_swizzle(kb, h, b);                      // grid (key blocks, H, B)
    const size_t rowbase = (size_t)b * L;
    const int k0 = kb * ABL_KB, nkeys = min(ABL_KB, Lp - k0);       // padded keys of this block (multiple of 16)
    {   // the block's K / V slices: 256 rows x 4 float4 each = 1024 items per tensor
        const int row = tid >> 2, c4 = (tid & 3) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (k0 + row < L) {
            const size_t off = (rowbase + k0 + row) * D + h * HD + c4;
            kv = *reinterpret_cast<const float4*>(K + off);
            vv = *reinterpret_cast<const float4*>(V + off);
        }
        *reinterpret_cast<float4*>(&Ks[row * AB_KST + c4]) = kv;
        *reinterpret_cast<float4*>(&Vs[row * AB_KST + c4]) = vv;
        if (tid < ABL_KB) Mb[tid] = attn_key_bias(mask, rowbase, k0, tid, L);
    }
    const int ki = lane & 15, g = lane >> 4;
    const float scale = AttnHead<HD>::scale;
    f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    const int keyl = 16 * w + ki;               // key inside the block
    const bool has_keys = 16 * w < nkeys;
    const uint32_t hb = (uint32_t)(((size_t)(b + b_off) * H + h) * L);
    float4 kf = make_float4(0.f, 0.f, 0.f, 0.f), vf = kf;
    float mb = MASK_VALUE;
    // rows of the next pass: requested a pass ahead (threads 0-255: one float4 of Q, dA and att each)
    float4 nq, na, no;
    float nl = 0.f;
    auto fetch = [&](int qb) {
        const int row = qb + (tid >> 2), c4 = (tid & 3) * 4;
        nq = make_float4(0.f, 0.f, 0.f, 0.f); na = nq; no = nq; nl = 0.f;
        if (tid < 256 && row < L) {
            const size_t off = (rowbase + row) * D + h * HD + c4;
            nq = *reinterpret_cast<const float4*>(Q + off);
            na = *reinterpret_cast<const float4*>(dr + off);
            no = *reinterpret_cast<const float4*>(att + off);
            if ((tid & 3) == 0) nl = lse[((size_t)b * H + h) * L + row];
        }
    };
    auto stage = [&](int qb) {                  // (the previous pass' readers are behind a barrier)
        if (tid < 256) {
            const int rl = tid >> 2, c4 = (tid & 3) * 4;
            float4 av = na;
            if (d3.thresh && qb + rl < L) {     // r = drop3(att) + x  (:183-184)
                const uint32_t base = (uint32_t)((rowbase + qb + rl) * D + h * HD + c4);
                av.x *= drop_mul(d3, base); av.y *= drop_mul(d3, base + 1);
                av.z *= drop_mul(d3, base + 2); av.w *= drop_mul(d3, base + 3);
            }
            *reinterpret_cast<float4*>(&Qs[rl * AB_KST + c4]) = nq;
            *reinterpret_cast<float4*>(&As[rl * AB_KST + c4]) = av;
            {
                uint32_t h0, m0, l0, h1, m1, l1;
                const int po = af_kp(rl, c4 >> 3) + (c4 & 7);
                split3(nq.x, nq.y, h0, m0, l0); split3(nq.z, nq.w, h1, m1, l1);
                *reinterpret_cast<u32x2_t*>(Qp + po) = u32x2_t{h0, h1};
                *reinterpret_cast<u32x2_t*>(Qp + QPL + po) = u32x2_t{m0, m1};
                *reinterpret_cast<u32x2_t*>(Qp + 2 * QPL + po) = u32x2_t{l0, l1};
                split3(av.x, av.y, h0, m0, l0); split3(av.z, av.w, h1, m1, l1);
                *reinterpret_cast<u32x2_t*>(Ap + po) = u32x2_t{h0, h1};
                *reinterpret_cast<u32x2_t*>(Ap + QPL + po) = u32x2_t{m0, m1};
                *reinterpret_cast<u32x2_t*>(Ap + 2 * QPL + po) = u32x2_t{l0, l1};
            }
            float dsum = av.x * no.x + av.y * no.y + av.z * no.z + av.w * no.w;     // D_q = dA . O (= sum_k dP_k P_k)
            dsum += lane_xor1(dsum);
            dsum += lane_xor2(dsum);
            if ((tid & 3) == 0) { Ds[rl] = dsum; Ls[rl] = nl; }
        }
    };
    fetch(0);
    __syncthreads();
    // B operands of the wave's key tile (column = key ki; k group g < 2: dims 8 g .. of the first term of the pair, g >= 2: dims 8 (g - 2) .. of the
    // second):  [Q_h | Q_m] x [K_h | K_h] + [Q_h | Q_l] x [K_m | K_h] + [Q_h | Q_m] x [K_l | K_m], the same with (dA, V)
    u32x4_t bk1, bk2, bk3, bv1, bv2, bv3;
#pragma unroll
    for (int e = 0; e < 4; ++e) { bk1[e] = bk2[e] = bk3[e] = bv1[e] = bv2[e] = bv3[e] = 0u; }
    if (has_keys) {
        mb = Mb[keyl];
        auto split8 = [&](const float* row, u32x4_t& b1, u32x4_t& b2, u32x4_t& b3) {
            const float4 xa = *reinterpret_cast<const float4*>(row + 8 * (g & 1)), xb = *reinterpret_cast<const float4*>(row + 8 * (g & 1) + 4);
            uint32_t th[4], tm[4], tl[4];
            split3(xa.x, xa.y, th[0], tm[0], tl[0]); split3(xa.z, xa.w, th[1], tm[1], tl[1]);
            split3(xb.x, xb.y, th[2], tm[2], tl[2]); split3(xb.z, xb.w, th[3], tm[3], tl[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e) { b1[e] = th[e]; b2[e] = g < 2 ? tm[e] : th[e]; b3[e] = g < 2 ? tl[e] : tm[e]; }
        };
        split8(&Ks[keyl * AB_KST], bk1, bk2, bk3);
        split8(&Vs[keyl * AB_KST], bv1, bv2, bv3);
    }
    const int pa1 = (g < 2 ? 0 : 1) * QPL, pa2 = (g < 2 ? 0 : 2) * QPL;        // A operands: planes (h | m) and (h | l) by k group
    for (int qb = 0; qb < Lp; qb += AB_QP) {
        const int qe = min(qb + AB_QP, Lp);
        stage(qb);
        if (qb + AB_QP < Lp) fetch(qb + AB_QP);
        __syncthreads();
        if (has_keys) {
            for (int qt = qb; qt < qe; qt += 16) {
                const int ql0 = qt - qb;
                const int ao = af_kp(ql0 + ki, g & 1);
                const u32x4_t q1 = *reinterpret_cast<const u32x4_t*>(Qp + pa1 + ao), q2 = *reinterpret_cast<const u32x4_t*>(Qp + pa2 + ao);
                const u32x4_t a1 = *reinterpret_cast<const u32x4_t*>(Ap + pa1 + ao), a2 = *reinterpret_cast<const u32x4_t*>(Ap + pa2 + ao);
                f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                sc = mfma16_bf16(q1, bk3, sc);          // hl + mm (small terms first)
                dp = mfma16_bf16(a1, bv3, dp);
                sc = mfma16_bf16(q2, bk2, sc);          // hm + lh
                dp = mfma16_bf16(a2, bv2, dp);
                sc = mfma16_bf16(q1, bk1, sc);          // hh + mh
                dp = mfma16_bf16(a1, bv1, dp);
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
                    const float p = __expf(sc[r] * scale + mb - Ls[ql]);
                    const float m2 = m2v[r];
                    const float pd = p * m2;
                    const float ds = p * (dp[r] * m2 - Ds[ql]) * scale;
                    if (DQ) dSs[ql * AB_DSP + keyl] = ds;
                    dv = __builtin_amdgcn_mfma_f32_16x16x4f32(As[ql * AB_KST + ki], pd, dv, 0, 0, 0);
                    dk = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[ql * AB_KST + ki], ds, dk, 0, 0, 0);
                }
            }
        }
        if constexpr (DQ) {
        __syncthreads();                        // dS of this pass complete
        const int qt2 = qb + 16 * (w & 3), kr = w >> 2;
        f32x4 dqs = {0.f, 0.f, 0.f, 0.f};
        if (qt2 < qe) {
            f32x4 dq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* kp = Ks + g * AB_KST + ki;
            const float* sp = dSs + (16 * (w & 3) + ki) * AB_DSP + g;
            for (int kk = 16 * kr; kk < nkeys; kk += 64) {
                float ka[4], sb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { ka[i] = kp[(kk + 4 * i) * AB_KST]; sb[i] = sp[kk + 4 * i]; }
#pragma unroll
                for (int i = 0; i < 4; ++i) dq[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[i], sb[i], dq[i], 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) dqs[c] = (dq[0][c] + dq[1][c]) + (dq[2][c] + dq[3][c]);
        }
        __syncthreads();                        // every wave has read its dS rows: the buffer becomes the exchange area
        float4* xq = reinterpret_cast<float4*>(dSs);          // [3 residues][4 query tiles][64 lanes]
        if (kr > 0) xq[((kr - 1) * 4 + (w & 3)) * 64 + lane] = make_float4(dqs[0], dqs[1], dqs[2], dqs[3]);
        __syncthreads();
        if (kr == 0 && qt2 < qe) {
            const float4 p1 = xq[(0 * 4 + w) * 64 + lane], p2 = xq[(1 * 4 + w) * 64 + lane], p3 = xq[(2 * 4 + w) * 64 + lane];
            const int q = qt2 + ki;
            if (q < L)
                *reinterpret_cast<float4*>(dQ + (size_t)kb * slab + (rowbase + q) * D + h * HD + 4 * g) =
                    make_float4(((dqs[0] + p1.x) + p2.x) + p3.x, ((dqs[1] + p1.y) + p2.y) + p3.y,
                                ((dqs[2] + p1.z) + p2.z) + p3.z, ((dqs[3] + p1.w) + p2.w) + p3.w);
        }
        }
        __syncthreads();                        // dS buffer, Qs / As / Ls / Ds free for the next pass
    }
    if (has_keys && k0 + keyl < L) {
        const size_t off = (rowbase + k0 + keyl) * D + h * HD + 4 * g;
        *reinterpret_cast<float4*>(dK + off) = make_float4(dk[0], dk[1], dk[2], dk[3]);
        *reinterpret_cast<float4*>(dV + off) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    }
}
int attn_bwd_dq_slabs(int L) { const int Lp = (L + 15) & ~15; return Lp <= 256 ? 1 : (Lp + ABL_KB - 1) / ABL_KB; }
template <bool PAIR, bool DQ> static void attn_bwd_long_go(const AttnArgs& a, int blocks, hipStream_t s) {
    dynamic_lds_optin<k_attn_bwd_long<PAIR, DQ>>(abl_lds(), "k_attn_bwd_long");
    VSL_LAUNCH((k_attn_bwd_long<PAIR, DQ>), dim3(blocks, a.H, a.B), dim3(1024), abl_lds(), s, a.Q, a.K, a.V, a.att, a.dr, a.lse, a.mask, a.dQ, a.dK, a.dV,
               a.L, a.H, a.b_off, (size_t)a.B * a.L * D, a.d2, a.d3);
}
void launch_attn_h16_bwd(const AttnArgs& a, bool dq, hipStream_t s) {
    const int Lp = (a.L + 15) & ~15, blocks = (Lp + ABL_KB - 1) / ABL_KB;
    if (!dq) return attn_bwd_long_go<true, false>(a, blocks, s);       // L > ATTN_SLAB_MAX_L: dK / dV per key block, dQ from k_attn_dq
    if (Lp <= 128) {
        dynamic_lds_optin<k_attn_bwd_fused<128>>(ab_lds<128>(), "k_attn_bwd_fused<128>");
        VSL_LAUNCH(k_attn_bwd_fused<128>, dim3(a.H, a.B), dim3(1024), ab_lds<128>(), s, a.Q, a.K, a.V, a.att, a.dr, a.lse, a.mask, a.dQ, a.dK, a.dV,
                   a.L, a.H, a.b_off, a.d2, a.d3);
        static int left = 3;
        if (stamps::enabled() && a.L > 64) stamps::report("attn_bwd_fused: stage-issue | landed+sync | pass-0 phase1 | sync | phase2 | sync | pass 1 + final", 8, s, left);
        return;
    }
    // 128 < L <= 256 as ONE 256-key block of the L > 256 kernel (S and dP on the bf16 pipe, Q / dA streamed in passes of 64) with the element hashes
    // of the L <= 256 forward.  (k_attn_bwd_fused<256>, 152 KB of LDS, served these lengths until round 6: +0.8 % on configs[2] / [3].)
    // L > 256: one pass over S / dP per key block of 256; dQ arrives as attn_bwd_dq_slabs(L) partial slabs (k_qkv_bwd adds them)
    if (Lp <= 256) attn_bwd_long_go<false, true>(a, 1, s);
    else attn_bwd_long_go<true, true>(a, blocks, s);
}

}  // namespace vsl
