// CQAttention forward kernels of the VSLNet hot path (gfx950): the trilinear score and both softmaxes, WeightedPool, CQConcatenate, HighLightLayer and
// the gating (backward: kernels_cq_bwd.hip -- a unit of its own because the forward kernels compile to other code beside the backward ones).
// Every kernel cites the reference lines it reproduces (layers_t7.py unless noted).  Activations are row-major (B*L, 128) fp32.
#include "common.hpp"
#include "launch.hpp"
#include <algorithm>

namespace vsl {

// =========================================================================================================
// a10  CQAttention (:208-243), three kernels.
//  (1) k_cq_score: trilinear score on dropped-out C, Q (:237-242) for a 32-row tile + row softmax over the
//      query words (:225).  Writes raw score S (B,T,Lq) and S_row (B,T,Lq).
//  (2) k_cq_col  : per sample: column softmax over clips (:226) -> S_col (B,T,Lq);  M = S_col^T C (Lq,128)
//      (re-association of (S_row S_col^T) C = S_row (S_col^T C): O(T Lq d) instead of O(T^2 d), fp32 rounding only);
//      plus a11's WeightedPool (:253-259) and the per-sample bias  pb = W2 pooled + b  of CQConcatenate (:268-274).
//  (3) k_cq_out  : c2q = S_row Q, q2c = S_row M, concat [C, c2q, C*c2q, C*q2c] (:231) -> Conv1D 4d->d (:232).
// =========================================================================================================
// a11's WeightedPool (:253-259) and the pooled half of CQConcatenate's Conv1D (:268-274) for one sample: alpha, pooled, pb = W2 pooled + b.  Query-side only;
// one 256-thread workgroup.  al: [128], pl: [128] floats of LDS.
// qsrc: first row of the sample's query in Qf / qmask (b Lq, or qidx[b] Lq when the queries are a resident encoding: vsl_localize_pairs); what is written stays at b.
__device__ __forceinline__ void cq_pool_body(const float* __restrict__ Qf, const float* __restrict__ qmask, const CqPoolArgs& cp, int b, size_t qsrc, int Lq, float* al, float* pl) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t qrow = (size_t)b * Lq;
    const float* pool_w = cp.pool_w; const float* Wcat = cp.Wcat; const float* bcat = cp.bcat;
    float* alpha = cp.alpha; float* pooled = cp.pooled; float* pb = cp.pb;
    // ---- WeightedPool: alpha = softmax_j(Q[j].w + mask) ; pooled = sum_j alpha_j Q[j]
    for (int jj = w; jj < Lq; jj += 4) {
        const float* row = Qf + (qsrc + jj) * D;
        const float d = wave_sum(row[lane] * pool_w[lane] + row[lane + 64] * pool_w[lane + 64]);
        if (lane == 0) al[jj] = d + (1.f - qmask[qsrc + jj]) * MASK_VALUE;
    }
    __syncthreads();
    if (w == 0) {                              // a lane owns words lane and lane + 64
        const float v0 = lane < Lq ? al[lane] : -3.0e38f, v1 = lane + 64 < Lq ? al[lane + 64] : -3.0e38f;
        const float mx = wave_max(fmaxf(v0, v1));
        const float e0 = lane < Lq ? __expf(v0 - mx) : 0.f, e1 = lane + 64 < Lq ? __expf(v1 - mx) : 0.f;
        const float inv = 1.0f / wave_sum(e0 + e1);
        // (alpha, pooled: read by the backward alone -- null in inference mode)
        if (lane < Lq) { al[lane] = e0 * inv; if (alpha) alpha[qrow + lane] = e0 * inv; }
        if (lane + 64 < Lq) { al[lane + 64] = e1 * inv; if (alpha) alpha[qrow + lane + 64] = e1 * inv; }
    }
    __syncthreads();
    if (tid < D) {
        float acc = 0.f;
        for (int j0 = 0; j0 < Lq; j0 += 8) {        // eight rows in flight; same summation order as one row at a time
            float qv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) qv[u] = Qf[(qsrc + min(j0 + u, Lq - 1)) * D + tid];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (j0 + u < Lq) acc += al[j0 + u] * qv[u];
        }
        pl[tid] = acc;
        if (pooled) pooled[(size_t)b * D + tid] = acc;
    }
    __syncthreads();
    // ---- pb[o] = sum_c Wcat[o][128 + c] * pooled[c] + bcat[o]     (second half of the 2d -> d Conv1D); 8 lanes per row
    for (int o = tid >> 3; o < D; o += 32) {
        const int sub = tid & 7;
        const float* wr = Wcat + (size_t)o * 2 * D + D + sub * 4;
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 wv = *reinterpret_cast<const float4*>(wr + 32 * q);
            const float4 pv = *reinterpret_cast<const float4*>(pl + sub * 4 + 32 * q);
            d += wv.x * pv.x + wv.y * pv.y + wv.z * pv.z + wv.w * pv.w;
        }
        d = grp8_sum(d);
        if (sub == 0) pb[(size_t)b * D + o] = d + bcat[o];
    }
}

// VIDX (the three CQAttention kernels): the context of sample b is video vidx[b] of a resident (N, T, 128) encoding (vsl_localize) -- the READS of C
// go through the index, one scalar load per workgroup; everything written stays at sample b.  VIDX = false: C is (B, T, 128), `vidx` is not read.
// QIDX (the pairs instantiations, vsl_localize_pairs: always together with VIDX): the query of sample b is query qidx[b] of a resident (Q, Lq, 128)
// encoding with its (Q, Lq) mask -- the READS of Qf and qmask go through the index the same way.  QIDX = false: `qidx` is not read.
template <int NU, bool VIDX, bool QIDX>   // NU: words per lane of the row softmax: 8 (Lq <= 64), 12 (<= 96) or 16 (<= MAX_LQ = 128)
__global__ __launch_bounds__(256) void k_cq_score(const float* __restrict__ C, const float* __restrict__ Qf,
                                                  const float* __restrict__ qmask, const float* __restrict__ w4C,
                                                  const float* __restrict__ w4Q, const float* __restrict__ w4mlu,
                                                  float* __restrict__ S, float* __restrict__ Srow, int T, int Lq, int b_off,
                                                  Drop dc, Drop dq, CqPoolArgs cp, const int* __restrict__ vidx, const int* __restrict__ qidx) {
    // cp.pool_w != nullptr: ONE extra workgroup per sample (blockIdx.x = number of tiles) runs the WeightedPool / pooled-bias path (the column kernel
    // is folded into k_cq_out then: launch_cq_out)
    if (cp.pool_w && blockIdx.x == gridDim.x - 1) {          // (block-uniform)
        extern __shared__ __attribute__((aligned(16))) float psm[];
        const int pb = blockIdx.y;
        cq_pool_body(Qf, qmask, cp, pb, QIDX ? (size_t)qidx[pb] * Lq : (size_t)pb * Lq, Lq, psm, psm + 128);
        return;
    }
    // S[i][j] = Cd[i].w4C + Qd[j].w4Q + (Cd[i] * w4mlu).Qd[j]   (:233-243) on a 32-clip tile; Cd / Qd = dropped-out C / Q.
    // The trilinear term is a 32 x 32 MFMA tile per 32 query words with K = 128 split over the four waves (partial tiles
    // summed in wave order through LDS); the two rank-1 terms and the row softmax use 8 lanes per row.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NTJ = (Lq + 31) >> 5, PJ = 32 * NTJ + 1;
    float* Cs = smem;                         // [32][LDP]  Cd, then Cd * w4mlu
    float* Qs = Cs + TILE_M * LDP;            // [32 NTJ][LDP]  Qd (rows >= Lq zero)
    float* s0 = Qs + 32 * NTJ * LDP;          // [32]
    float* s1 = s0 + TILE_M;                  // [32 NTJ]
    float* Pp = s1 + 32 * NTJ;                // [4][32][PJ] per-wave partial tiles
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, hh = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * TILE_M;
    const size_t crow = (size_t)b * T, qrow = (size_t)b * Lq;
    const size_t vrow = VIDX ? (size_t)vidx[b] * T : crow;      // first row of this sample's context in C
    const size_t qsrc = QIDX ? (size_t)qidx[b] * Lq : qrow;     // ... of its query in Qf / qmask
    {   // one batch of 16-byte loads for both tiles, dropout applied on the way into LDS
        float4 cv[4], qv[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256, rr = e >> 5, c = (e & 31) * 4;
            const int t = min(t0 + rr, T - 1);
            cv[q] = *reinterpret_cast<const float4*>(C + (vrow + t) * D + c);
        }
        auto load_q = [&](int q0) {               // query rows 8 q0 .. : 8 float4 per thread (64 words) per pass
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = tid + (q0 + q) * 256, j = e >> 5, c = (e & 31) * 4;
                qv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q0 + q < 4 * NTJ) qv[q] = *reinterpret_cast<const float4*>(Qf + (qsrc + min(j, Lq - 1)) * D + c);
            }
        };
        auto store_q = [&](int q0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (q0 + q < 4 * NTJ) {
                    const int e = tid + (q0 + q) * 256, j = e >> 5, c = (e & 31) * 4;
                    float4 v = qv[q];
                    if (j < Lq) {
                        if (dq.thresh) {
                            const uint32_t base = (uint32_t)(((b + b_off) * Lq + j) * D + c);
                            v.x *= drop_keep_scale(dq, base); v.y *= drop_keep_scale(dq, base + 1);
                            v.z *= drop_keep_scale(dq, base + 2); v.w *= drop_keep_scale(dq, base + 3);
                        }
                    } else v = make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4*>(&Qs[j * LDP + c]) = v;
                }
            }
        };
        load_q(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256, rr = e >> 5, c = (e & 31) * 4;
            const int t = t0 + rr;
            float4 v = cv[q];
            if (t < T) {
                if (dc.thresh) {
                    const uint32_t base = (uint32_t)(((b + b_off) * T + t) * D + c);
                    v.x *= drop_keep_scale(dc, base); v.y *= drop_keep_scale(dc, base + 1);
                    v.z *= drop_keep_scale(dc, base + 2); v.w *= drop_keep_scale(dc, base + 3);
                }
            } else v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&Cs[rr * LDP + c]) = v;
        }
        store_q(0);
        for (int q0 = 8; q0 < 4 * NTJ; q0 += 8) { load_q(q0); store_q(q0); }     // queries beyond 64 words (ActivityNet: up to 82)
    }
    __syncthreads();
    {   // s0[i] = Cd[i] . w4C ; s1[j] = Qd[j] . w4Q ; then Cd *= w4mlu in place.  8 lanes per row, 32 rows per pass.
        const int sub = tid & 7, rr = tid >> 3;
        float4 wc[4], wq[4], wm[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wc[k] = *reinterpret_cast<const float4*>(w4C + sub * 4 + 32 * k);
            wq[k] = *reinterpret_cast<const float4*>(w4Q + sub * 4 + 32 * k);
            wm[k] = *reinterpret_cast<const float4*>(w4mlu + sub * 4 + 32 * k);
        }
        float d = 0.f;
        float* crp = Cs + rr * LDP + sub * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 v = *reinterpret_cast<const float4*>(crp + 32 * k);
            d += v.x * wc[k].x + v.y * wc[k].y + v.z * wc[k].z + v.w * wc[k].w;
            v.x *= wm[k].x; v.y *= wm[k].y; v.z *= wm[k].z; v.w *= wm[k].w;
            *reinterpret_cast<float4*>(crp + 32 * k) = v;
        }
        d = grp8_sum(d);
        if (sub == 0) s0[rr] = d;
        for (int jb = 0; jb < 32 * NTJ; jb += 32) {
            const float* qrp = Qs + (jb + rr) * LDP + sub * 4;
            float e = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v = *reinterpret_cast<const float4*>(qrp + 32 * k);
                e += v.x * wq[k].x + v.y * wq[k].y + v.z * wq[k].z + v.w * wq[k].w;
            }
            e = grp8_sum(e);
            if (sub == 0) s1[jb + rr] = e;
        }
    }
    __syncthreads();
    for (int nb = 0; nb < NTJ; nb += 2) {   // trilinear term: wave w contracts channels 32w .. 32w+31 ; two 32-word tiles per pass
        f32x16 acc[2];
        zero_acc(acc);
        const int i = lane & 31;
        const float* arow = Cs + i * LDP + 4 * hh;
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            const int kb = 4 * w + kq;
            const float4 av = *reinterpret_cast<const float4*>(arow + kb * 8);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                if (nb + nt < NTJ) {
                    const float4 bv = *reinterpret_cast<const float4*>(Qs + (32 * (nb + nt) + i) * LDP + kb * 8 + 4 * hh);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[nt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
            if (nb + nt < NTJ) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Pp[(w * TILE_M + acc_row(r, lane)) * PJ + 32 * (nb + nt) + i] = acc[nt][r];
            }
    }
    __syncthreads();
    {   // raw score + row softmax over the query words (dim=2, :225) with the query mask; 8 lanes per clip
        const int sub = tid & 7, rr = tid >> 3;
        const int t = t0 + rr;
        float raw[NU], v[NU];
        float mx = -3.0e38f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int j = sub + 8 * u;
            raw[u] = 0.f; v[u] = -3.0e38f;
            if (j < Lq) {
                raw[u] = Pp[rr * PJ + j] + Pp[(TILE_M + rr) * PJ + j] + Pp[(2 * TILE_M + rr) * PJ + j] + Pp[(3 * TILE_M + rr) * PJ + j] +
                         s0[rr] + s1[j];
                v[u] = raw[u] + (1.f - qmask[qsrc + j]) * MASK_VALUE;
                mx = fmaxf(mx, v[u]);
            }
        }
        mx = fmaxf(mx, lane_xor1(mx)); mx = fmaxf(mx, lane_xor2(mx)); mx = fmaxf(mx, lane_half_mirror(mx));
        float sm = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) { v[u] = (sub + 8 * u < Lq) ? __expf(v[u] - mx) : 0.f; sm += v[u]; }
        const float inv = 1.0f / grp8_sum(sm);
        if (t < T) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = sub + 8 * u;
                if (j < Lq) { S[(crow + t) * Lq + j] = raw[u]; Srow[(crow + t) * Lq + j] = v[u] * inv; }
            }
        }
    }
}
template <int NU, bool VIDX, bool QIDX = false> static void cq_score_go(const CqFwdArgs& a, const char* name, hipStream_t s) {
    const int NTJ = (a.Lq + 31) / 32;
    const size_t shm = (size_t)((TILE_M + 32 * NTJ) * LDP + TILE_M + 32 * NTJ + 4 * TILE_M * (32 * NTJ + 1)) * sizeof(float);
    const dim3 grid((a.T + TILE_M - 1) / TILE_M + (a.fold ? 1 : 0), a.B);
    dynamic_lds_optin<k_cq_score<NU, VIDX, QIDX>>(shm, name);
    VSL_LAUNCH((k_cq_score<NU, VIDX, QIDX>), grid, dim3(256), shm, s, a.C, a.Qf, a.qmask, a.w4C, a.w4Q, a.w4mlu, a.S, a.Srow, a.T, a.Lq, a.b_off, a.dc, a.dq,
               a.fold ? a.pool : CqPoolArgs{}, a.vidx, a.qidx);
}
void launch_cq_score(const CqFwdArgs& a, hipStream_t s) {
    if (a.qidx) {        // (vsl_localize_pairs: both indices)
        if (a.Lq <= 64) cq_score_go<8, true, true>(a, "k_cq_score<8, true, true>", s);
        else if (a.Lq <= 96) cq_score_go<12, true, true>(a, "k_cq_score<12, true, true>", s);
        else cq_score_go<16, true, true>(a, "k_cq_score<16, true, true>", s);
        return;
    }
    if (a.Lq <= 64) { if (a.vidx) cq_score_go<8, true>(a, "k_cq_score<8, true>", s); else cq_score_go<8, false>(a, "k_cq_score<8>", s); }
    else if (a.Lq <= 96) { if (a.vidx) cq_score_go<12, true>(a, "k_cq_score<12, true>", s); else cq_score_go<12, false>(a, "k_cq_score<12>", s); }
    else { if (a.vidx) cq_score_go<16, true>(a, "k_cq_score<16, true>", s); else cq_score_go<16, false>(a, "k_cq_score<16>", s); }
}

template <bool VIDX, bool QIDX>
__global__ __launch_bounds__(256) void k_cq_col(const float* __restrict__ C, const float* __restrict__ Qf,
                                                const float* __restrict__ S, const float* __restrict__ cmask,
                                                const float* __restrict__ qmask, const float* __restrict__ pool_w,
                                                const float* __restrict__ Wcat, const float* __restrict__ bcat,
                                                float* __restrict__ Scol, float* __restrict__ Mpart, float* __restrict__ alpha,
                                                float* __restrict__ pooled, float* __restrict__ pb, int T, int Lq,
                                                const int* __restrict__ vidx, const int* __restrict__ qidx) {
    // Tile-parallel: workgroup = (32-clip tile, sample).  The column-softmax statistics need every clip of the sample, so
    // each workgroup recomputes them from the sample's whole score matrix (T x Lq floats, L2-resident, all 256 threads);
    // it then writes its S_col tile and the per-tile partial of M = S_col^T C (MFMA, gemm_tn); k_cq_out adds the partials.
    // One EXTRA workgroup per sample (blockIdx.x = number of tiles) runs the small WeightedPool / pooled-bias path beside the tiles
    // (it used to ride on tile 0 and made that workgroup the critical one).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LQ1 = Lq + 1;
    float* Cs = smem;                         // [32][LDP]  C tile
    float* Ss = Cs + TILE_M * LDP;            // [32][LQ1]  S_col tile (+ slack for the 32-wide over-read of gemm_tn)
    constexpr int JS = 128;                   // word stride of the statistics arrays (Lq <= MAX_LQ <= 128)
    float* redm = Ss + TILE_M * LQ1 + 72;     // [8][JS] partial column maxima
    float* reds = redm + 8 * JS;              // [8][JS] partial column sums
    float* cmax = reds + 8 * JS;              // [JS]
    float* cinv = cmax + JS;                  // [JS]
    float* al = cinv + JS;                    // [JS]
    float* pl = al + JS;                      // [128]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, tl = blockIdx.x, t0 = tl * TILE_M, ntile = gridDim.x - 1;
    const size_t crow = (size_t)b * T, qrow = (size_t)b * Lq;
    if (tl < ntile) {                           // block-uniform
    load_tile128(Cs, C + (VIDX ? (size_t)vidx[b] * T : crow) * D, t0, TILE_M, T);
    // ---- column statistics over all T clips: thread = (word j, part); a part walks clips part, part + np, ... -- eight loads in
    //      flight at a time (one load per trip of a data-dependent loop costs a full memory latency per clip)
    const int JW = Lq <= 32 ? 32 : Lq <= 64 ? 64 : 128, np = 256 / JW;
    const int j = tid & (JW - 1), part = tid / JW;
    auto walk = [&](auto&& fold) {
        if (j >= Lq) return;
        for (int i0 = part; i0 < T; i0 += 8 * np) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * np, T - 1);
                v[u] = S[(crow + i) * Lq + j] + (1.f - cmask[crow + i]) * MASK_VALUE;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) if (i0 + u * np < T) fold(v[u]);
        }
    };
    {
        float mx = -3.0e38f;
        walk([&](float v) { mx = fmaxf(mx, v); });
        redm[part * JS + j] = mx;
    }
    __syncthreads();
    float gm = -3.0e38f;
    for (int q = 0; q < np; ++q) gm = fmaxf(gm, redm[q * JS + j]);
    {
        float sm = 0.f;
        walk([&](float v) { sm += __expf(v - gm); });
        reds[part * JS + j] = sm;
    }
    __syncthreads();
    if (tid < JW) {
        float sm = 0.f;
        for (int q = 0; q < np; ++q) sm += reds[q * JS + j];
        cmax[j] = gm;
        cinv[j] = 1.0f / sm;
    }
    if (tid < 72) Ss[TILE_M * LQ1 + tid] = 0.f;          // finite values where gemm_tn over-reads
    __syncthreads();
    // ---- S_col tile (:226-227), written out and kept in LDS with a zero pad column
    for (int e = tid; e < TILE_M * LQ1; e += 256) {
        const int i = e / LQ1, jj = e - i * LQ1;
        float v = 0.f;
        if (jj < Lq && t0 + i < T) {
            const size_t o = (crow + t0 + i) * Lq + jj;
            v = __expf(S[o] + (1.f - cmask[crow + t0 + i]) * MASK_VALUE - cmax[jj]) * cinv[jj];
            if (Scol) Scol[o] = v;         // (null in inference mode)
        }
        Ss[e] = v;
    }
    __syncthreads();
    // ---- partial of M[j][c] = sum_t S_col[t][j] C[t][c] over this tile's clips
    {
        float* mp = Mpart + (size_t)(b * ntile + tl) * Lq * D;
        const int col = 32 * w + (lane & 31);
        const int NTJ = (Lq + 31) >> 5;
        for (int nt = 0; nt < NTJ; ++nt) {
            f32x16 acc[1];
            zero_acc(acc);
            gemm_tn_p<1, TILE_M>(Ss, LQ1, 32 * nt, Cs, LDP, 32 * w, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = 32 * nt + acc_row(r, lane);
                if (jj < Lq) mp[(size_t)jj * D + col] = acc[0][r];
            }
        }
    }
    return;
    }
    cq_pool_body(Qf, qmask, CqPoolArgs{pool_w, Wcat, bcat, alpha, pooled, pb}, b, QIDX ? (size_t)qidx[b] * Lq : qrow, Lq, al, pl);
}
bool cq_col_folds(int T, int Lq) { return T <= 4 * TILE_M && Lq <= 32; }      // (k_cq_out's fold: at most four tiles per sample, one 32-word tile of M)
void launch_cq_col(const CqFwdArgs& a, hipStream_t s) {
    const size_t shm = (size_t)(TILE_M * LDP + TILE_M * (a.Lq + 1) + 72 + 2 * 8 * 128 + 3 * 128 + D) * sizeof(float);
    const dim3 grid((a.T + TILE_M - 1) / TILE_M + 1, a.B);
    const CqPoolArgs& p = a.pool;
    auto go = [&](auto kern) {
        VSL_LAUNCH(kern, grid, dim3(256), shm, s, a.C, a.Qf, a.S, a.vmask, a.qmask, p.pool_w, p.Wcat, p.bcat, a.Scol, a.Mpart, p.alpha, p.pooled, p.pb, a.T, a.Lq,
                   a.vidx, a.qidx);
    };
    if (a.qidx) go(k_cq_col<true, true>);        // (vsl_localize_pairs: both indices)
    else if (a.vidx) go(k_cq_col<true, false>); else go(k_cq_col<false, false>);
}

// CQConcatenate + HighLightLayer + gating (a11 / a12, VSLNet_t7.py:60) ride on the same kernel (row-local on the tile just produced)
struct CqCatFuse {
    const float *W1pack, *pb, *wh, *bh, *vmask;
    float *f2, *hscore, *gated;
    // the column kernel folded in (T <= 128, Lq <= 32: launch_cq_out): every workgroup computes its SAMPLE's column-softmax statistics and
    // M = S_col^T C over all (at most four) tiles itself instead of summing k_cq_col's per-tile partials -- 4 x 16 KB of L2 reads and four small
    // MFMA products per workgroup against a launch + a kernel boundary on the dependent chain.  S == nullptr: off.
    const float *S, *cmask;
    float* Scol;
};
template <bool VIDX, bool QIDX>
__global__ __launch_bounds__(256) void k_cq_out(const float* __restrict__ C, const float* __restrict__ Qf,
                                                const float* __restrict__ Srow, const float* __restrict__ Mpart,
                                                float* __restrict__ M, const float* __restrict__ Wpack,
                                                const float* __restrict__ bias, float* __restrict__ cat_out,
                                                float* __restrict__ out, int T, int Lq, CqCatFuse cf,
                                                const int* __restrict__ vidx, const int* __restrict__ qidx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LQ1 = Lq + 1;
    // Lq > CQ_BIG_LQ: M lives where the concat tile will be written (it is dead by then, behind one extra barrier): 101 instead of 167 KB
    const bool big = Lq > CQ_BIG_LQ;
    const int cat_floats = big ? max(TILE_M * CATP, Lq * LDP) : TILE_M * CATP;
    float* Cat = smem;                        // [32][CATP]
    float* Cs = Cat + cat_floats;             // [32][LDP]
    float* Ms = big ? Cat : Cs + TILE_M * LDP;   // [Lq][LDP]   M = S_col^T C, summed here from k_cq_col's per-tile partials
    float* Ss = Cs + TILE_M * LDP + (big ? 0 : Lq * LDP);   // [32][LQ1]   S_row tile, zero pad column
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, hh = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * TILE_M, ntile = gridDim.x;
    const size_t crow = (size_t)b * T, qrow = (size_t)b * Lq;
    const size_t vrow = VIDX ? (size_t)vidx[b] * T : crow;      // first row of this sample's context in C
    const size_t qsrc = QIDX ? (size_t)qidx[b] * Lq : qrow;     // ... of its query in Qf
    BFrag<1, 16> bf;
    load_tile128(Cs, C + vrow * D, t0, TILE_M, T);
    if (cf.S) {                                // (block-uniform) k_cq_col's work for the whole sample, in the concat tile's LDS (dead until the concat)
        constexpr int JS = 128;
        float* Ct = Cat;                       // [32][LDP]   C tile of the pass
        float* Sc = Ct + TILE_M * LDP;         // [32][LQ1] + 72   S_col tile (+ slack for the 32-wide over-read of gemm_tn)
        float* redm = Sc + TILE_M * LQ1 + 72;  // [8][JS]
        float* reds = redm + 8 * JS;           // [8][JS]
        float* cmax = reds + 8 * JS;           // [JS]
        float* cinv = cmax + JS;               // [JS]
        const float* S = cf.S;
        const float* cmask = cf.cmask;
        const int JW = 32, np = 256 / JW;      // (Lq <= 32 here)
        const int j = tid & (JW - 1), part = tid / JW;
        auto walk = [&](auto&& fold) {
            if (j >= Lq) return;
            for (int i0 = part; i0 < T; i0 += 8 * np) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = min(i0 + u * np, T - 1);
                    v[u] = S[(crow + i) * Lq + j] + (1.f - cmask[crow + i]) * MASK_VALUE;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) if (i0 + u * np < T) fold(v[u]);
            }
        };
        {
            float mx = -3.0e38f;
            walk([&](float v) { mx = fmaxf(mx, v); });
            redm[part * JS + j] = mx;
        }
        __syncthreads();
        float gm = -3.0e38f;
        for (int q = 0; q < np; ++q) gm = fmaxf(gm, redm[q * JS + j]);
        {
            float sm = 0.f;
            walk([&](float v) { sm += __expf(v - gm); });
            reds[part * JS + j] = sm;
        }
        __syncthreads();
        if (tid < JW) {
            float sm = 0.f;
            for (int q = 0; q < np; ++q) sm += reds[q * JS + j];
            cmax[j] = gm;
            cinv[j] = 1.0f / sm;
        }
        if (tid < 72) Sc[TILE_M * LQ1 + tid] = 0.f;          // finite values where gemm_tn over-reads
        f32x16 macc[1];
        zero_acc(macc);
        for (int tl = 0; tl < ntile; ++tl) {                 // M[j][c] = sum over ALL clips of the sample, tile by tile (k_cq_col's order within a tile)
            const int tt0 = tl * TILE_M;
            __syncthreads();                                 // the previous pass' product is done with Ct / Sc ; cmax / cinv are written
            load_tile128(Ct, C + vrow * D, tt0, TILE_M, T);
            for (int e = tid; e < TILE_M * LQ1; e += 256) {
                const int i = e / LQ1, jj = e - i * LQ1;
                float v = 0.f;
                if (jj < Lq && tt0 + i < T) {
                    const size_t o = (crow + tt0 + i) * Lq + jj;
                    v = __expf(S[o] + (1.f - cmask[crow + tt0 + i]) * MASK_VALUE - cmax[jj]) * cinv[jj];
                    if (cf.Scol && tl == (int)blockIdx.x) cf.Scol[o] = v;       // this workgroup's own tile (saved for the backward; null in inference mode)
                }
                Sc[e] = v;
            }
            __syncthreads();
            gemm_tn_p<1, TILE_M>(Sc, LQ1, 0, Ct, LDP, 32 * w, macc);
        }
        {
            const int colm = 32 * w + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = acc_row(r, lane);
                if (jj < Lq) {
                    Ms[jj * LDP + colm] = macc[0][r];
                    if (M && blockIdx.x == 0) M[(qrow + jj) * D + colm] = macc[0][r];     // saved for the backward (null in inference mode)
                }
            }
        }
        __syncthreads();                                     // Cat's region is free for the concat again ; Ms is complete
    } else
    for (int e = tid; e < Lq * (D / 4); e += 256) {
        const int j = e >> 5, c4 = (e & 31) * 4;
        float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < ntile; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(Mpart + ((size_t)(b * ntile + t) * Lq + j) * D + c4);
            sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
        }
        *reinterpret_cast<float4*>(Ms + j * LDP + c4) = sm;
        if (M && blockIdx.x == 0) *reinterpret_cast<float4*>(M + (qrow + j) * D + c4) = sm;     // saved for the backward
    }
    for (int e = tid; e < TILE_M * LQ1; e += 256) {
        const int rr = e / LQ1, j = e - rr * LQ1;
        Ss[e] = (j < Lq && t0 + rr < T) ? Srow[(crow + t0 + rr) * Lq + j] : 0.f;
    }
    bfrag_load(bf, Wpack, D, 32 * w, 0, 0, 4 * D / 8);
    __syncthreads();
    // c2q = S_row Q, q2c = S_row M (:229-230) on the matrix cores (K = Lq, wave = 32 channels), then the concat tile (:231)
    const int col = 32 * w + (lane & 31);
    {
        f32x16 c2q[1], q2c[1];
        zero_acc(c2q);
        zero_acc(q2c);
        const float* sa = Ss + (lane & 31) * LQ1 + hh;
        for (int jc = 0; jc < Lq; jc += 16) {
            float sv[8], qv[8], mv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = jc + 2 * u + hh;
                const bool ok = j < Lq;
                sv[u] = ok ? sa[jc + 2 * u] : 0.f;
                qv[u] = ok ? Qf[(qsrc + j) * D + col] : 0.f;
                mv[u] = ok ? Ms[j * LDP + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (jc + 2 * u < Lq) {
                    c2q[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u], qv[u], c2q[0], 0, 0, 0);
                    q2c[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u], mv[u], q2c[0], 0, 0, 0);
                }
            }
        }
        if (big) __syncthreads();                  // block-uniform: every wave is done with M before the concat tile overwrites it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, lane);
            const float cv = Cs[rr * LDP + col];
            float* o = Cat + rr * CATP;
            o[col] = cv;
            o[D + col] = c2q[0][r];
            o[2 * D + col] = cv * c2q[0][r];
            o[3 * D + col] = cv * q2c[0][r];
        }
    }
    __syncthreads();
    if (cat_out)                                   // saved: A operand (R, 512) of the cqa_linear weight gradient
        for (int e = tid; e < TILE_M * D; e += 256) {
            const int rr = e >> 7, c4 = (e & 127) * 4;
            if (t0 + rr < T)
                *reinterpret_cast<float4*>(cat_out + (crow + t0 + rr) * 4 * D + c4) = *reinterpret_cast<const float4*>(&Cat[rr * CATP + c4]);
        }
    f32x16 acc[1];
    zero_acc(acc);
    gemm32p<1, 16>(Cat, CATP, 4 * D, Wpack, D, 32 * w, 0, acc, bf);
    BFrag<1, 16> bf2;                              // weights of the fused CQConcatenate GEMM: in flight during the epilogue
    bfrag_load(bf2, cf.W1pack, D, 32 * w, 0, 0, D / 8);
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lane);
        const int t = t0 + row;
        const float v = acc[0][r] + bv;
        if (out && t < T) out[(crow + t) * D + col] = v;      // (f1: null in inference mode, like f2 below)
        Cs[row * LDP + col] = t < T ? v : 0.f;     // the C tile is dead: A operand of the next GEMM
    }
    __syncthreads();
    // ---- f2 = f1 W1^T + (W2 pooled + b) ; h = sigmoid(mask_logits(f2 . w_h + b_h)) ; gated = f2 * h
    float* Fs = Cat;                               // [32][LDP] (the concat tile is dead after the barrier above)
    float* hs = Ss;                                // [32]
    f32x16 a2[1];
    zero_acc(a2);
    gemm32p<1, 16>(Cs, LDP, D, cf.W1pack, D, 32 * w, 0, a2, bf2);
    {
        const float pbv = cf.pb[(size_t)b * D + col];
#pragma unroll
        for (int r = 0; r < 16; ++r) Fs[acc_row(r, lane) * LDP + col] = a2[0][r] + pbv;
    }
    __syncthreads();
    {
        const int rr = tid >> 3, sub = tid & 7;
        const float* row = Fs + rr * LDP + sub * 4;
        float d = 0.f;
#pragma unroll
        for (int jq = 0; jq < 4; ++jq) {
            const float4 fv = *reinterpret_cast<const float4*>(row + 32 * jq);
            const float4 wv = *reinterpret_cast<const float4*>(cf.wh + sub * 4 + 32 * jq);
            d += fv.x * wv.x + fv.y * wv.y + fv.z * wv.z + fv.w * wv.w;
        }
        d = grp8_sum(d);
        if (sub == 0) {
            const int t = t0 + rr;
            float hv = 0.f;
            if (t < T) {
                const float lg = d + cf.bh[0] + (1.f - cf.vmask[crow + t]) * MASK_VALUE;      // mask_logits (:286)
                hv = 1.0f / (1.0f + __expf(-lg));
                cf.hscore[crow + t] = hv;
            }
            hs[rr] = hv;
        }
    }
    __syncthreads();
    for (int e = tid; e < TILE_M * 32; e += 256) {
        const int rr = e >> 5, c = (e & 31) * 4;
        const int t = t0 + rr;
        if (t < T) {
            const float4 v = *reinterpret_cast<const float4*>(&Fs[rr * LDP + c]);
            const float hv = hs[rr];
            if (cf.f2) *reinterpret_cast<float4*>(cf.f2 + (crow + t) * D + c) = v;
            *reinterpret_cast<float4*>(cf.gated + (crow + t) * D + c) = make_float4(v.x * hv, v.y * hv, v.z * hv, v.w * hv);
        }
    }
}
template <bool VIDX, bool QIDX = false> static void cq_out_go(const CqFwdArgs& a, const char* name, hipStream_t s) {
    const int T = a.T, Lq = a.Lq;
    const size_t shm = (Lq > CQ_BIG_LQ ? (size_t)(std::max(TILE_M * CATP, Lq * LDP) + TILE_M * LDP + TILE_M * (Lq + 1) + 32)
                                       : (size_t)(TILE_M * CATP + TILE_M * LDP + Lq * LDP + TILE_M * (Lq + 1) + 32)) * sizeof(float);
    const dim3 grid((T + TILE_M - 1) / TILE_M, a.B);
    const CqCatFuse cf{a.W1pack, a.pool.pb, a.wh, a.bh, a.vmask, a.f2, a.hscore, a.gated, a.fold ? a.S : nullptr, a.fold ? a.vmask : nullptr, a.fold ? a.Scol : nullptr};
    dynamic_lds_optin<k_cq_out<VIDX, QIDX>>(shm, name);
    VSL_LAUNCH((k_cq_out<VIDX, QIDX>), grid, dim3(256), shm, s, a.C, a.Qf, a.Srow, a.Mpart, a.M, a.Wcqa, a.bcqa, a.cat, a.f1, T, Lq, cf, a.vidx, a.qidx);
}
void launch_cq_out(const CqFwdArgs& a, hipStream_t s) {
    if (a.qidx) cq_out_go<true, true>(a, "k_cq_out<true, true>", s);        // (vsl_localize_pairs: both indices)
    else if (a.vidx) cq_out_go<true>(a, "k_cq_out<true>", s); else cq_out_go<false>(a, "k_cq_out", s);
}

// the (N, T) clip mask of a resident encoding expanded to one row per query: out[b][t] = vmask[vidx[b]][t] (vsl_localize; the predictor, head and
// LSTM kernels index their mask by sample)
__global__ __launch_bounds__(256) void k_vmask_gather(const float* __restrict__ vmask, const int* __restrict__ vidx, float* __restrict__ out, int T) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) out[(size_t)b * T + t] = vmask[(size_t)vidx[b] * T + t];
}
void launch_vmask_gather(const float* vmask, const int* vidx, float* out, int B, int T, hipStream_t s) {
    VSL_LAUNCH(k_vmask_gather, dim3((T + 255) / 256, B), dim3(256), 0, s, vmask, vidx, out, T);
}

}  // namespace vsl
