// The attention core's dispatch (launch_attn_fwd / launch_attn_bwd of launch.hpp: head count -> unit, attn.hpp) and the query-major dQ kernel of
// long videos (1024 < L <= MAX_L) for head sizes 16, 32 and 8 (num_heads 8, 4 and 16; 128 and 64: k_attn_wide_dq of kernels_attn_wide.hip).
//   a8 (:174-182)  S = Q K^T / sqrt(hd) + (1 - mask[key]) * -1e30 ; P = softmax ; O = drop(P) V
// The key-major kernels (k_attn_bwd_long, k_attn_hd_bwd) run one workgroup per 256-key block; their dQ is a partial over that block, so up to
// L = 1024 it leaves them as attn_bwd_dq_slabs(L) (R, 128) slabs that k_qkv_bwd adds.  That workspace and the extra reads grow as L^2 / 256.
// Above 1024 the key-major kernels compute dK / dV only (their DQ = false instantiation) and k_attn_dq computes dQ in full, once, into slab 0:
// the dQ workspace is one (R, 128) tensor whatever L is.  VSL_ATTN_DQ_SLABS=1 keeps the slab scheme at every L (comparison only).
#include "attn.hpp"

namespace vsl {

constexpr int ADQ_KB = 128;         // keys staged per block
template <int HDV> struct AttnDq : AttnHead<HDV> {
    static_assert(HDV == 8 || HDV == 16 || HDV == 32, "head sizes 8, 16 and 32");
    static constexpr int NJ = ADQ_KB * AttnHead<HDV>::F4 / 256;      // float4 per thread and tensor of a staged block
};
template <int HDV> constexpr size_t attn_dq_lds() { return (size_t)(2 * ADQ_KB * AttnDq<HDV>::KST + ADQ_KB) * sizeof(float); }

// ---------------------------------------------------------------------------------------------------------
// k_attn_dq.  Workgroup = (64 queries, head, sample), wave = 16 queries; lane (qi, g) owns query column qi of the transposed tiles
// S^T = K Q^T and dP^T = V dA^T (keys 16 t + 4 g + r), as in the forward (k_attn_fwd).  Its query's Q, dA = dr * m3, LSE and
// Delta = dA . O stay in registers for the whole kernel.  K / V head slices are staged in LDS per block of 128 keys; the next block's rows
// travel in registers while the current one is worked on.  Per 16-key tile:
//   P^T = exp(S^T c + bias - LSE), the forward's key-pair dropout decisions (both keys of a pair sit in one lane), dS^T = P^T (dP^T m2 - Delta) c,
//   dQ^T[dd][q] += K^T[dd][key] dS^T[key][q]   (A = K from LDS, B = dS^T straight from the accumulator registers).
// Every product on the fp32-input MFMA (v_mfma_f32_16x16x4_f32); dQ accumulates in registers in key order and is written once: no atomics,
// fixed summation order.  Rows past L: zero Q / dA and LSE 0 give dS = 0; keys past L carry the mask bias (P = 0).
// ---------------------------------------------------------------------------------------------------------
template <int HDV>
__global__ __launch_bounds__(256) void k_attn_dq(const float* __restrict__ Q, const float* __restrict__ K,
                                                 const float* __restrict__ V, const float* __restrict__ att,
                                                 const float* __restrict__ dr, const float* __restrict__ lse,
                                                 const float* __restrict__ mask, float* __restrict__ dQ, int L, int H,
                                                 int b_off, Drop d2, Drop d3) {
    using C = AttnDq<HDV>;
    constexpr int KST = C::KST, NC = C::NC, NT = C::NT, F4 = C::F4, NJ = C::NJ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;                 // [128][KST]
    float* Vs = Ks + ADQ_KB * KST;    // [128][KST]
    float* Mb = Vs + ADQ_KB * KST;    // [128] additive key bias
    const int Lp = (L + 15) & ~15;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int qbk, h, b;
    xcd_swizzle(qbk, h, b);                        // grid (query blocks, H, B)
    const size_t rowbase = (size_t)b * L;
    const int qi = lane & 15, g = lane >> 4;
    const int q = qbk * 64 + w * 16 + qi;
    const bool qok = q < L;
    const float scale = C::scale;
    // B operands of S^T and dP^T: Q[q][g NC + c] and dA[q][g NC + c]
    float qa[NC], aa[NC], oa[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) qa[c] = aa[c] = oa[c] = 0.f;
    float lq = 0.f;
    if (qok) {
        const size_t off = (rowbase + q) * D + h * HDV + g * NC;
        load_nc<NC>(Q + off, qa);
        load_nc<NC>(dr + off, aa);
        load_nc<NC>(att + off, oa);
        if (d3.thresh) {                           // r = drop3(att) + x  (:183-184): element-keyed, as the key-major kernels stage it
#pragma unroll
            for (int c = 0; c < NC; ++c) aa[c] *= drop_mul(d3, (uint32_t)(off + c));
        }
        lq = lse[((size_t)b * H + h) * L + q];
    }
    float dl = 0.f;                                // Delta_q = dA . O (= sum_k dP_k P_k): the four k groups of the query in a fixed order
#pragma unroll
    for (int c = 0; c < NC; ++c) dl = fmaf(aa[c], oa[c], dl);
    dl += __shfl_xor(dl, 16);
    dl += __shfl_xor(dl, 32);
    const uint32_t qrow = (uint32_t)(((size_t)(b + b_off) * H + h) * L + q);       // dropout of the probabilities as the forward drew it: key pairs (L > 1024)
    const uint32_t prow = attn_drop_pair_row(qrow, L);
    const bool dropon = d2.thresh != 0u;
    f32x4 dq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 pk[NJ], pv[NJ];
    float pm = 0.f;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int e = tid + 256 * j, key = k0 + e / F4, c4 = (e % F4) * 4;
            pk[j] = make_float4(0.f, 0.f, 0.f, 0.f); pv[j] = pk[j];
            if (key < L) {
                pk[j] = *reinterpret_cast<const float4*>(K + (rowbase + key) * D + h * HDV + c4);
                pv[j] = *reinterpret_cast<const float4*>(V + (rowbase + key) * D + h * HDV + c4);
            }
        }
        if (tid < ADQ_KB) pm = attn_key_bias(mask, rowbase, k0, tid, L);
    };
    fetch(0);
    for (int k0 = 0; k0 < Lp; k0 += ADQ_KB) {
        const int nk = min(ADQ_KB, Lp - k0);
        if (k0) __syncthreads();                   // every wave is done with the previous block
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int e = tid + 256 * j, kl = e / F4, c4 = (e % F4) * 4;
            *reinterpret_cast<float4*>(&Ks[kl * KST + c4]) = pk[j];
            *reinterpret_cast<float4*>(&Vs[kl * KST + c4]) = pv[j];
        }
        if (tid < ADQ_KB) Mb[tid] = pm;
        __syncthreads();
        if (k0 + ADQ_KB < Lp) fetch(k0 + ADQ_KB);
        for (int kt = 0; kt < nk; kt += 16) {
            // S^T = K Q^T and dP^T = V dA^T: A[i = key][k = g] = K[key][g NC + c] (resp. V), B[k = g][j = query] = Q[q][g NC + c] (resp. dA)
            float ka[NC], va[NC];
            load_nc<NC>(&Ks[(kt + qi) * KST + g * NC], ka);
            load_nc<NC>(&Vs[(kt + qi) * KST + g * NC], va);
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[c], qa[c], sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c], aa[c], dp, 0, 0, 0);
            }
            const float4 mb = *reinterpret_cast<const float4*>(&Mb[kt + 4 * g]);
            const float mbr[4] = {mb.x, mb.y, mb.z, mb.w};
            float m2v[4] = {1.f, 1.f, 1.f, 1.f};
            if (dropon) attn_drop_pair4(d2, prow, k0 + kt + 4 * g, m2v);
            float ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(sc[r] * scale + mbr[r] - lq);
                ds[r] = p * (dp[r] * m2v[r] - dl) * scale;
            }
            // dQ^T[dd][q] += K[key][dd] dS^T[key][q]: A[i = dd][k = key 4 g + r] = K, B[k][j = q] = ds[r] of this lane (one MFMA per r)
            const bool in = HDV >= 16 || qi < HDV;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float kd = in ? Ks[(kt + 4 * g + r) * KST + 16 * j + (qi & (HDV - 1))] : 0.f;
                    dq[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kd, ds[r], dq[j], 0, 0, 0);
                }
        }
    }
    if (qok) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (HDV >= 16 || g < HDV / 4)          // dQ^T rows dd = 16 j + 4 g + r
                *reinterpret_cast<float4*>(dQ + (rowbase + q) * D + h * HDV + 16 * j + 4 * g) = make_float4(dq[j][0], dq[j][1], dq[j][2], dq[j][3]);
    }
}

bool attn_dq_query_major(int L) {
    static const bool slabs = switch_on("VSL_ATTN_DQ_SLABS", false);
    return L > ATTN_SLAB_MAX_L && !slabs;
}
int attn_dq_slabs(int L) { return attn_dq_query_major(L) ? 1 : attn_bwd_dq_slabs(L); }

void launch_attn_fwd(const AttnArgs& a, hipStream_t s) {
    if (a.H <= 2) launch_attn_wide_fwd(a, s);          // head sizes 128 / 64 (kernels_attn_wide.hip)
    else if (a.H != 8) launch_attn_hd_fwd(a, s);       // head sizes 32 / 8 (kernels_attn_hd.hip)
    else launch_attn_h16_fwd(a, s);                    // head size 16 (kernels_attn_h16.hip)
}

void launch_attn_bwd(const AttnArgs& a, hipStream_t s) {
    const bool qmaj = attn_dq_query_major(a.L);
    if (a.H <= 2) return launch_attn_wide_bwd(a, qmaj, s);     // their own dK / dV and query-major dQ kernels
    if (a.H != 8) launch_attn_hd_bwd(a, !qmaj, s);
    else launch_attn_h16_bwd(a, !qmaj, s);
    if (!qmaj) return;
    attn_for_head_size<16, 32, 8>(a.H, [&](auto hd) {
        constexpr int HDV = decltype(hd)::value;
        dynamic_lds_optin<k_attn_dq<HDV>>(attn_dq_lds<HDV>(), "k_attn_dq");
        VSL_LAUNCH(k_attn_dq<HDV>, dim3((a.L + 63) / 64, a.H, a.B), dim3(256), attn_dq_lds<HDV>(), s, a.Q, a.K, a.V, a.att, a.dr, a.lse, a.mask, a.dQ,
                   a.L, a.H, a.b_off, a.d2, a.d3);
    });
}

}  // namespace vsl
