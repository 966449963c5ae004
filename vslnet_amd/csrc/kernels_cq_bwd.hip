// CQAttention backward kernels of the VSLNet hot path (gfx950): gating + HighLightLayer + CQConcatenate, then CQAttention + WeightedPool as four
// tile-parallel kernels (forward: kernels_cq.hip).  The reference has no hand-written backward: each kernel names the forward lines (layers_t7.py)
// it differentiates.  Parameter gradients leave as per-tile / per-sample PARTIAL SLABS that k_reduce (kernels_params.hip) sums.
#include "common.hpp"
#include "launch.hpp"
#include "tile_bodies.hpp"
#include "stamps.hpp"
#include <type_traits>

namespace vsl {

// =========================================================================================================
// a11 + a12 backward: gated = f2 * h ; h = sigmoid(mask_logits(f2 . wh + bh)) ; f2 = f1 W1^T + pb[b]
//   dgated = dg0 + dg1 + dg2 (two heads + predictor encoder input) ; dh_loss from the highlight loss.
// =========================================================================================================
__global__ __launch_bounds__(256) void k_cqcat_bwd(CqcatBwdArgs a, int R) {
    __shared__ __attribute__((aligned(16))) float Gs[TILE_M * LDP];     // dgated -> df2
    __shared__ __attribute__((aligned(16))) float Fs[TILE_M * LDP];     // f2
    __shared__ float dlg[TILE_M];
    cqcat_bwd_tile(a, nullptr, Gs, Fs, dlg, blockIdx.x * TILE_M, R);
}
void launch_cqcat_bwd(const CqcatBwdArgs& a, int R, hipStream_t s) {
    VSL_LAUNCH(k_cqcat_bwd, dim3((R + TILE_M - 1) / TILE_M), dim3(256), 0, s, a, R);
}

// =========================================================================================================
// a10 / a11 backward (CQAttention :208-243, WeightedPool / CQConcatenate bias :246-274) as FOUR tile-parallel kernels.
// Grid = (32-clip tiles, samples) for A, B, C -- every reduction over the clips of a sample goes through small per-tile
// partials that the next kernel sums in its prologue -- and one workgroup per sample for the tiny finalise D.
//   A: dcat = df1 Wcqa ; split into dC(direct), dc2q, dq2c ; dS_row + row-softmax backward -> dSr ;
//      per-tile partials of dM = S_row^T dq2c and dQ(c2q) = S_row^T dc2q
//   B: dM = sum of partials ; dS_col = C dM^T (-> scratch) ; per-tile partial of the column-softmax dot
//   C: dS = dSr + S_col * (dS_col - dot) ; dC total ; per-tile partials of colsum(dS), dQ(trilinear), colsum(df2),
//      and the w4C / w4mlu parameter slabs
//   D: dQ total (+ WeightedPool / pooled-bias path), w4Q / pool / W2 / bias slabs
// =========================================================================================================
template <bool VIDX>
__global__ __launch_bounds__(256) void k_cq_bwd_a(CqBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T = a.T, Lq = a.Lq, LQ1 = Lq + 1;
    const int NTJ = (Lq + 31) >> 5, PJ = 32 * NTJ + 1;      // 32-wide query-word tiles of the small MFMA products
    float* Dc = smem;                          // [32][CATP] grad wrt the concat tile
    float* Gs = Dc + TILE_M * CATP;            // [32][LDP]  df1 tile, later C tile
    float* Ss = Gs + TILE_M * LDP;             // [32][LQ1]  S_row, pad column zeroed (+ slack for the 32-wide over-read)
    float* Sd = Ss + TILE_M * LQ1 + 8;         // [32][LQ1]  dS_row
    float* Pp = Sd + TILE_M * LQ1 + 64;        // [4][32][PJ] per-wave partial sums of dS_row ; Lq > CQ_BIG_LQ: [32][PJ], one wave per word tile
    const bool big = Lq > CQ_BIG_LQ;            // NTJ = 4 then
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, tl = blockIdx.x, t0 = tl * TILE_M, ntile = gridDim.x;
    const size_t crow = (size_t)b * T, qrow = (size_t)b * Lq;
    STAMP(0);
    load_tile128(Gs, a.df1 + crow * D, t0, TILE_M, T);
    for (int e = tid; e < TILE_M * LQ1; e += 256) {
        const int i = e / LQ1, j = e - i * LQ1;
        Ss[e] = (j < Lq && t0 + i < T) ? a.Srow[(crow + t0 + i) * Lq + j] : 0.f;
    }
    if (tid < 72) Sd[TILE_M * LQ1 - 8 + tid] = 0.f;          // finite values wherever the over-reads of Ss / Sd land
    BFrag<4, 4> bf;
    bfrag_load(bf, a.WcqaT, 4 * D, 32 * w, D, 0, D / 8);
    __syncthreads();
    STAMP(1);
    f32x16 acc[4];
    zero_acc(acc);
    gemm32p<4, 4>(Gs, LDP, D, a.WcqaT, 4 * D, 32 * w, D, acc, bf);
    const int col = 32 * w + (lane & 31), hh = lane >> 5;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Dc[acc_row(r, lane) * CATP + t * D + col] = acc[t][r];
    STAMP(2);
    __syncthreads();
    load_tile128(Gs, a.C + (VIDX ? (size_t)a.vidx[b] * T : crow) * D, t0, TILE_M, T);      // Gs now holds the C tile
    // recompute c2q = S_row Q and q2c = S_row M (:229-230) on the matrix cores: K = Lq, wave = 32 output channels
    f32x16 c2q[1], q2c[1];
    zero_acc(c2q);
    zero_acc(q2c);
    {
        const float* sa = Ss + (lane & 31) * LQ1 + hh;
        for (int jc = 0; jc < Lq; jc += 16) {              // 8 k-steps per chunk: all loads first, then the MFMAs
            float sv[8], qv[8], mv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = jc + 2 * u + hh;
                const bool ok = j < Lq;
                sv[u] = ok ? sa[jc + 2 * u] : 0.f;
                qv[u] = ok ? a.Qf[(qrow + j) * D + col] : 0.f;
                mv[u] = ok ? a.M[(qrow + j) * D + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (jc + 2 * u < Lq) {
                    c2q[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u], qv[u], c2q[0], 0, 0, 0);
                    q2c[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u], mv[u], q2c[0], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
    STAMP(3);
    // product-rule split of :231 in the accumulator layout (lane = channel, 16 rows)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lane);
        float* d = Dc + rr * CATP;
        const float cv = Gs[rr * LDP + col];
        const float d0 = d[col], d1 = d[D + col], d2 = d[2 * D + col], d3 = d[3 * D + col];
        d[D + col] = d1 + d2 * cv;             // dc2q, kept in LDS: dS dots and the dM / dQ partials below
        d[3 * D + col] = d3 * cv;              // dq2c
        if (t0 + rr < T) a.dC[(crow + t0 + rr) * D + col] = d0 + d2 * c2q[0][r] + d3 * q2c[0][r];
    }
    __syncthreads();
    STAMP(4);
    {   // dS_row[i][j] = dc2q[i] . Q[j] + dq2c[i] . M[j]: a 32 x 32 MFMA tile per 32 query words, K = 256 split over
        // the four waves (wave w: channels 32w .. 32w+31 of both halves), partial tiles summed in wave order through LDS
        const int i = lane & 31;
        if (big) {                                              // wave w = word tile w over the whole K = 256: no partial tiles
            f32x16 dsw[1];
            zero_acc(dsw);
            const int j = 32 * w + i;
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const float* src = part ? a.M : a.Qf;
                const float* arow = Dc + i * CATP + (part ? 3 * D : D) + 4 * hh;
                for (int kb = 0; kb < D / 8; kb += 4) {
                    float4 bq4[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        bq4[q] = j < Lq ? *reinterpret_cast<const float4*>(src + (qrow + j) * D + (kb + q) * 8 + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 av = *reinterpret_cast<const float4*>(arow + (kb + q) * 8);
                        dsw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bq4[q].x, dsw[0], 0, 0, 0);
                        dsw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bq4[q].y, dsw[0], 0, 0, 0);
                        dsw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bq4[q].z, dsw[0], 0, 0, 0);
                        dsw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bq4[q].w, dsw[0], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) Pp[acc_row(r, lane) * PJ + 32 * w + i] = dsw[0][r];
        } else
        for (int nb = 0; nb < NTJ; nb += 2) {                   // two 32-word tiles per pass (one pass up to 64 query words)
        f32x16 ds[2];
        zero_acc(ds);
        float4 bq[2][2][4];                                  // [part][nt][kq]: every B fragment is requested up front
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const float* src = part ? a.M : a.Qf;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int kq = 0; kq < 4; ++kq) {
                    const int j = 32 * (nb + nt) + i;
                    bq[part][nt][kq] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (nb + nt < NTJ && j < Lq)
                        bq[part][nt][kq] = *reinterpret_cast<const float4*>(src + (qrow + j) * D + (4 * w + kq) * 8 + 4 * hh);
                }
        }
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const float* arow = Dc + i * CATP + (part ? 3 * D : D) + 4 * hh;
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
                const float4 av = *reinterpret_cast<const float4*>(arow + (4 * w + kq) * 8);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    if (nb + nt < NTJ) {
                        const float4 bv = bq[part][nt][kq];
                        ds[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, ds[nt], 0, 0, 0);
                        ds[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, ds[nt], 0, 0, 0);
                        ds[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, ds[nt], 0, 0, 0);
                        ds[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, ds[nt], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
            if (nb + nt < NTJ) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Pp[(w * TILE_M + acc_row(r, lane)) * PJ + 32 * (nb + nt) + i] = ds[nt][r];
            }
        }
    }
    // per-tile partials on the matrix cores: dM_t[j][c] = sum_i Srow[i][j] dq2c[i][c] ; dQa_t[j][c] = sum_i Srow[i][j] dc2q[i][c]
    {
        float* p1 = a.P1 + ((size_t)(b * ntile + tl) * 2) * Lq * D;
        for (int nt = 0; nt < NTJ; ++nt) {
            f32x16 am[1], aq[1];
            zero_acc(am);
            zero_acc(aq);
            gemm_tn_p<1, TILE_M>(Ss, LQ1, 32 * nt, Dc + 3 * D, CATP, 32 * w, am);
            gemm_tn_p<1, TILE_M>(Ss, LQ1, 32 * nt, Dc + D, CATP, 32 * w, aq);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * nt + acc_row(r, lane);
                if (j < Lq) { p1[(size_t)j * D + col] = am[0][r]; p1[(size_t)(Lq + j) * D + col] = aq[0][r]; }
            }
        }
    }
    STAMP(5);
    __syncthreads();
    STAMP(6);
    if (tid < TILE_M) {                          // softmax backward over the query words (dim=2, :225), thread = clip
        const int t = t0 + tid;
        if (t < T) {
            const float* sr = Ss + tid * LQ1;
            float dot = 0.f;
            for (int j = 0; j < Lq; ++j) {
                const float g = big ? Pp[tid * PJ + j]
                                    : Pp[tid * PJ + j] + Pp[(TILE_M + tid) * PJ + j] + Pp[(2 * TILE_M + tid) * PJ + j] +
                                      Pp[(3 * TILE_M + tid) * PJ + j];
                Sd[tid * LQ1 + j] = g;
                dot += sr[j] * g;
            }
            for (int j = 0; j < Lq; ++j) a.dSr[(crow + t) * Lq + j] = sr[j] * (Sd[tid * LQ1 + j] - dot);
        }
    }
    STAMP(7);
}

// sums the per-tile partials of dM into LDS (dMs [Lq][LDP]); 8 loads in flight per thread
__device__ __forceinline__ void cq_sum_dM(float* dMs, const float* __restrict__ P1, int b, int ntile, int Lq) {
    for (int e = threadIdx.x; e < Lq * (D / 4); e += 256) {
        const int j = e >> 5, c4 = (e & 31) * 4;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < ntile; t += 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = t + u < ntile ? *reinterpret_cast<const float4*>(P1 + ((size_t)(b * ntile + t + u) * 2) * Lq * D + (size_t)j * D + c4)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        *reinterpret_cast<float4*>(dMs + j * LDP + c4) = s;
    }
}

template <bool VIDX>
__global__ __launch_bounds__(256) void k_cq_bwd_b(CqBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T = a.T, Lq = a.Lq, LQ1 = Lq + 1;
    const int NTJ = (Lq + 31) >> 5, PJ = 32 * NTJ + 1;
    float* dMs = smem;                         // [32 NTJ][LDP]  dM (rows >= Lq zero)
    float* Cs = dMs + 32 * NTJ * LDP;          // [32][LDP]
    float* St = Cs + TILE_M * LDP;             // [32][LQ1] S_col tile
    float* Pp = St + TILE_M * LQ1;             // [4][32][PJ] per-wave partial tiles of dS_col ; Lq > CQ_BIG_LQ: [32][PJ], one wave per word tile
    const bool big = Lq > CQ_BIG_LQ;            // NTJ = 4 then
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, hh = lane >> 5;
    const int b = blockIdx.y, tl = blockIdx.x, t0 = tl * TILE_M, ntile = gridDim.x;
    const size_t crow = (size_t)b * T;
    load_tile128(Cs, a.C + (VIDX ? (size_t)a.vidx[b] * T : crow) * D, t0, TILE_M, T);
    for (int e = tid; e < TILE_M * Lq; e += 256) {
        const int i = e / Lq, j = e - i * Lq;
        St[i * LQ1 + j] = t0 + i < T ? a.Scol[(crow + t0) * Lq + e] : 0.f;
    }
    cq_sum_dM(dMs, a.P1, b, ntile, Lq);
    for (int e = tid; e < (32 * NTJ - Lq) * (D / 4); e += 256)         // zero rows Lq .. 32 NTJ - 1 (B operand of the padded tile)
        *reinterpret_cast<float4*>(dMs + (Lq + (e >> 5)) * LDP + (e & 31) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (big) {                              // wave w = word tile w over the whole K = 128
        f32x16 accw[1];
        zero_acc(accw);
        const int i = lane & 31;
        const float* arow = Cs + i * LDP + 4 * hh;
        const float* brow = dMs + (32 * w + i) * LDP + 4 * hh;
#pragma unroll
        for (int kb = 0; kb < D / 8; ++kb) {
            const float4 av = *reinterpret_cast<const float4*>(arow + kb * 8);
            const float4 bv = *reinterpret_cast<const float4*>(brow + kb * 8);
            accw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, accw[0], 0, 0, 0);
            accw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, accw[0], 0, 0, 0);
            accw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, accw[0], 0, 0, 0);
            accw[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, accw[0], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Pp[acc_row(r, lane) * PJ + 32 * w + i] = accw[0][r];
    } else
    for (int nb = 0; nb < NTJ; nb += 2) {   // dS_col[i][j] = C[i] . dM[j]: 32 x 32 MFMA tile per 32 query words, K = 128 split over the waves
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
                    const float4 bv = *reinterpret_cast<const float4*>(dMs + (32 * (nb + nt) + i) * LDP + kb * 8 + 4 * hh);
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
    // sum the four partial tiles in wave order, write dS_col, and the per-tile partial of the column-softmax dot
    for (int e = tid; e < TILE_M * Lq; e += 256) {
        const int i = e / Lq, j = e - i * Lq;
        const float sv = big ? Pp[i * PJ + j]
                             : Pp[i * PJ + j] + Pp[(TILE_M + i) * PJ + j] + Pp[(2 * TILE_M + i) * PJ + j] + Pp[(3 * TILE_M + i) * PJ + j];
        Pp[i * PJ + j] = sv;                                                    // only this thread touches (i, j)
        if (t0 + i < T) a.dSs[(crow + t0) * Lq + e] = sv;
    }
    __syncthreads();
    if (tid < Lq) {
        float sacc = 0.f;
        for (int i = 0; i < TILE_M; ++i) sacc += Pp[i * PJ + tid] * St[i * LQ1 + tid];
        a.P2[(size_t)(b * ntile + tl) * Lq + tid] = sacc;
    }
}
template <bool VIDX>
__global__ __launch_bounds__(256) void k_cq_bwd_c(CqBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T = a.T, Lq = a.Lq, LQ1 = Lq + 1;
    float* dMs = smem;                         // [Lq][LDP]  dM
    const bool big = Lq > CQ_BIG_LQ;            // then the dropped-out Q is not staged: its one use reads memory and re-applies the mask
    float* Qds = dMs + Lq * LDP;               // [Lq][LDP]  dropped-out Q (as used by the trilinear score)
    float* Cs = Qds + (big ? 0 : Lq * LDP);    // [32][LDP]  C tile, later df2 tile
    float* Cd = Cs + TILE_M * LDP;             // [32][LDP]  dropped C tile
    float* St = Cd + TILE_M * LDP;             // [32][LQ1]  S_col tile
    float* Sg = St + TILE_M * LQ1 + 8;         // [32][LQ1]  dS tile (+ slack for the chunked over-read)
    float* csum = Sg + TILE_M * LQ1 + 8;       // [Lq]
    float* rsum = csum + Lq;                   // [32]
    float* v128 = rsum + TILE_M;               // [4][128]
    const int tid = threadIdx.x;
    const int b = blockIdx.y, tl = blockIdx.x, t0 = tl * TILE_M, ntile = gridDim.x;
    const size_t crow = (size_t)b * T, qrow = (size_t)b * Lq;
    // ---- prologue: tile loads + the cross-tile sums
    load_tile128(Cs, a.C + (VIDX ? (size_t)a.vidx[b] * T : crow) * D, t0, TILE_M, T);
    cq_sum_dM(dMs, a.P1, b, ntile, Lq);
    if (!big)
    for (int e = tid; e < Lq * D; e += 256) {
        const int j = e >> 7, cc = e & 127;
        Qds[j * LDP + cc] = a.Qf[(qrow + j) * D + cc] * drop_mul(a.dq, (uint32_t)(((b + a.b_off) * Lq + j) * D + cc));
    }
    if (tid < Lq) {
        float s = 0.f;
        for (int t = 0; t < ntile; ++t) s += a.P2[(size_t)(b * ntile + t) * Lq + tid];
        csum[tid] = s;
    }
    __syncthreads();
    for (int e = tid; e < TILE_M * LQ1; e += 256) {
        const int i = e / LQ1, j = e - i * LQ1;
        float g = 0.f, st = 0.f;
        if (j < Lq && t0 + i < T) {
            const size_t o = (crow + t0 + i) * Lq + j;
            st = a.Scol[o];
            g = a.dSr[o] + st * (a.dSs[o] - csum[j]);
        }
        St[e] = st;
        Sg[e] = g;
    }
    for (int e = tid; e < TILE_M * D; e += 256) {
        const int rr = e >> 7, cc = e & 127;
        const int t = t0 + rr;
        Cd[rr * LDP + cc] = t < T ? Cs[rr * LDP + cc] * drop_mul(a.dc, (uint32_t)(((b + a.b_off) * T + t) * D + cc)) : 0.f;
    }
    __syncthreads();
    if (tid < TILE_M) { float s = 0.f; for (int j = 0; j < Lq; ++j) s += Sg[tid * LQ1 + j]; rsum[tid] = s; }
    if (tid >= 64 && tid < 64 + Lq) {          // per-tile partial of colsum(dS)
        const int j = tid - 64;
        float s = 0.f;
        for (int i = 0; i < TILE_M; ++i) s += Sg[i * LQ1 + j];
        a.P3[(size_t)(b * ntile + tl) * Lq + j] = s;
    }
    __syncthreads();
    float acc_w4C = 0.f, acc_mlu = 0.f;
    const int w = tid >> 6, lane = tid & 63, hh = lane >> 5, col = 32 * w + (lane & 31);
    {
        // tq = dS Qd and tm = S_col dM (K = Lq) on the matrix cores; wave = 32 channels, accumulator layout lane = channel
        f32x16 tq[1], tm[1];
        zero_acc(tq);
        zero_acc(tm);
        const float* sgp = Sg + (lane & 31) * LQ1 + hh;
        const float* stp = St + (lane & 31) * LQ1 + hh;
        for (int jc = 0; jc < Lq; jc += 16) {
            float gv[8], sv[8], qv[8], mv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = jc + 2 * u + hh;
                const bool ok = j < Lq;
                gv[u] = ok ? sgp[jc + 2 * u] : 0.f;
                sv[u] = ok ? stp[jc + 2 * u] : 0.f;
                qv[u] = !ok ? 0.f : !big ? Qds[j * LDP + col]
                                          : a.Qf[(qrow + j) * D + col] * drop_mul(a.dq, (uint32_t)(((b + a.b_off) * Lq + j) * D + col));
                mv[u] = ok ? dMs[j * LDP + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (jc + 2 * u < Lq) {
                    tq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[u], qv[u], tq[0], 0, 0, 0);   // sum_j dS[i][j] Qd[j][c]
                    tm[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u], mv[u], tm[0], 0, 0, 0);   // sum_j Scol[i][j] dM[j][c]
                }
            }
        }
        const float wC = a.w4C[col], wM = a.w4mlu[col];
        float dcv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + acc_row(r, lane);
            dcv[r] = t < T ? a.dC[(crow + t) * D + col] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, lane);
            const int t = t0 + rr;
            const float cdv = Cd[rr * LDP + col];
            const float dcd = rsum[rr] * wC + wM * tq[0][r];      // grad wrt dropped-out C
            acc_w4C += rsum[rr] * cdv;
            acc_mlu += tq[0][r] * cdv;
            if (t < T) a.dC[(crow + t) * D + col] = dcv[r] + tm[0][r] + dcd * drop_mul(a.dc, (uint32_t)(((b + a.b_off) * T + t) * D + col));
        }
        // per-tile partial of dQ(trilinear)[j][c] = mask_q * w4mlu[c] * sum_i dS[i][j] Cd[i][c]
        float* p4 = a.P4 + (size_t)(b * ntile + tl) * Lq * D;
        const int NTJ = (Lq + 31) >> 5;
        for (int nt = 0; nt < NTJ; ++nt) {
            f32x16 pq[1];
            zero_acc(pq);
            gemm_tn_p<1, TILE_M>(Sg, LQ1, 32 * nt, Cd, LDP, 32 * w, pq);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * nt + acc_row(r, lane);
                if (j < Lq) p4[(size_t)j * D + col] = pq[0][r] * wM * drop_mul(a.dq, (uint32_t)(((b + a.b_off) * Lq + j) * D + col));
            }
        }
    }
    v128[hh * D + col] = acc_w4C;
    v128[2 * D + hh * D + col] = acc_mlu;
    __syncthreads();                           // (also: everyone is done with Cs)
    load_tile128(Cs, a.df2 + crow * D, t0, TILE_M, T);
    if (tid < D) {
        a.p_w4C[(size_t)(b * ntile + tl) * D + tid] = v128[tid] + v128[D + tid];
        a.p_w4mlu[(size_t)(b * ntile + tl) * D + tid] = v128[2 * D + tid] + v128[3 * D + tid];
    }
    __syncthreads();
    if (tid < D) {                             // per-tile partial of dpb[o] = sum_t df2[b, t, o]
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < TILE_M; ++i) s += Cs[i * LDP + tid];
        a.P5[(size_t)(b * ntile + tl) * D + tid] = s;
    }
}

__global__ __launch_bounds__(256) void k_cq_bwd_d(CqBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Lq = a.Lq, ntile = a.ntile;
    float* dQs = smem;                         // [Lq][LDP] dQ accumulator
    float* cs2 = dQs + Lq * LDP;               // [Lq] colsum(dS)
    float* sv = cs2 + Lq;                      // [Lq]
    float* v128 = sv + Lq;                     // [4][128]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const size_t qrow = (size_t)b * Lq;
    // Every cross-tile / cross-word sum below issues its loads in batches before the (ordered) additions: the kernel is one workgroup per
    // sample with nothing else to hide a memory round trip per loop iteration (82 % of its wave cycles were parked; 26 -> 18 us).  Round 2
    // measured the same change as a net loss because the query chain then took CUs from the (then critical) video chain; since round 3 the
    // query chain IS the critical tail of the backward.
    if (tid < Lq) {
        float s = 0.f;
        for (int t0 = 0; t0 < ntile; t0 += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = t0 + u < ntile ? a.P3[(size_t)(b * ntile + t0 + u) * Lq + tid] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        cs2[tid] = s;
    }
    if (tid < D) {                             // dpb[o] = sum over tiles of colsum(df2)
        float s = 0.f;
        for (int t0 = 0; t0 < ntile; t0 += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = t0 + u < ntile ? a.P5[(size_t)(b * ntile + t0 + u) * D + tid] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        v128[tid] = s;
        a.p_bcat[(size_t)b * D + tid] = s;
    }
    __syncthreads();
    // dQ = sum_tiles (dQ(c2q) + dQ(trilinear)) + colsum(dS)[j] * w4Q * mask_q
    for (int e = tid; e < Lq * (D / 4); e += 256) {
        const int j = e >> 5, c4 = (e & 31) * 4;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t0 = 0; t0 < ntile; t0 += 4) {
            float4 x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = min(t0 + u, ntile - 1);
                x[u] = *reinterpret_cast<const float4*>(a.P1 + ((size_t)(b * ntile + t) * 2 + 1) * Lq * D + (size_t)j * D + c4);
                y[u] = *reinterpret_cast<const float4*>(a.P4 + (size_t)(b * ntile + t) * Lq * D + (size_t)j * D + c4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (t0 + u < ntile) { s.x += x[u].x + y[u].x; s.y += x[u].y + y[u].y; s.z += x[u].z + y[u].z; s.w += x[u].w + y[u].w; }
        }
        const float4 wq = *reinterpret_cast<const float4*>(a.w4Q + c4);
        const uint32_t base = (uint32_t)(((b + a.b_off) * Lq + j) * D + c4);
        s.x += cs2[j] * wq.x * drop_mul(a.dq, base); s.y += cs2[j] * wq.y * drop_mul(a.dq, base + 1);
        s.z += cs2[j] * wq.z * drop_mul(a.dq, base + 2); s.w += cs2[j] * wq.w * drop_mul(a.dq, base + 3);
        *reinterpret_cast<float4*>(dQs + j * LDP + c4) = s;
    }
    if (tid < D) {                             // dw4Q[c] = sum_j colsum(dS)[j] * Qd[j][c]
        float s = 0.f;
        for (int j0 = 0; j0 < Lq; j0 += 8) {
            float qv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) qv[u] = a.Qf[(qrow + min(j0 + u, Lq - 1)) * D + tid];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < Lq) s += cs2[j0 + u] * qv[u] * drop_mul(a.dq, (uint32_t)(((b + a.b_off) * Lq + j0 + u) * D + tid));
        }
        a.p_w4Q[(size_t)b * D + tid] = s;
    }
    // ---- pooled-query path: pb = W2 pooled + bcat ; pooled = sum_j alpha_j Q[j] ; alpha = softmax(Q w + mask)
    for (int e = tid; e < D * D; e += 256)                // dW2[o][c] = dpb[o] * pooled[c]
        a.p_W2[(size_t)b * D * D + e] = v128[e >> 7] * a.pooled[(size_t)b * D + (e & 127)];
    {
        const int cc = tid & 127, hh = tid >> 7;
        float s8[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) s8[q] = 0.f;
        for (int o = hh * 64; o < hh * 64 + 64; o += 8) { // dpooled[c] = sum_o Wcat[o][128 + c] * dpb[o]
#pragma unroll
            for (int q = 0; q < 8; ++q) s8[q] += a.Wcat[(size_t)(o + q) * 2 * D + D + cc] * v128[o + q];
        }
        v128[2 * D + hh * D + cc] = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    }
    __syncthreads();
    if (tid < D) v128[D + tid] = v128[2 * D + tid] + v128[3 * D + tid];          // dpooled[c]
    __syncthreads();
    for (int j = w; j < Lq; j += 4) {                     // dalpha_j = dpooled . Q[j]
        const float* qr = a.Qf + (qrow + j) * D;
        const float d = wave_sum(qr[lane] * v128[D + lane] + qr[lane + 64] * v128[D + lane + 64]);
        if (lane == 0) sv[j] = d;
    }
    __syncthreads();
    if (w == 0) {
        const float a0 = lane < Lq ? a.alpha[qrow + lane] : 0.f, a1 = lane + 64 < Lq ? a.alpha[qrow + lane + 64] : 0.f;
        const float g0 = lane < Lq ? sv[lane] : 0.f, g1 = lane + 64 < Lq ? sv[lane + 64] : 0.f;
        const float dot = wave_sum(a0 * g0 + a1 * g1);
        if (lane < Lq) sv[lane] = a0 * (g0 - dot);        // dlogit_j
        if (lane + 64 < Lq) sv[lane + 64] = a1 * (g1 - dot);
    }
    __syncthreads();
    if (tid < D) {
        float s = 0.f;
        for (int j0 = 0; j0 < Lq; j0 += 8) {
            float qv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) qv[u] = a.Qf[(qrow + min(j0 + u, Lq - 1)) * D + tid];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < Lq) s += sv[j0 + u] * qv[u];
        }
        a.p_pool[(size_t)b * D + tid] = s;
    }
    for (int e = tid; e < Lq * D; e += 256) {
        const int j = e >> 7, cc = e & 127;
        a.dQ[(qrow + j) * D + cc] = dQs[j * LDP + cc] + a.alpha[qrow + j] * v128[D + cc] + sv[j] * a.pool_w[cc];
    }
}

void launch_cq_bwd(const CqBwdArgs& a0, int B, hipStream_t s) {
    CqBwdArgs a = a0;
    const int Lq = a.Lq, ntile = (a.T + TILE_M - 1) / TILE_M;
    a.ntile = ntile;
    const int npart = Lq > CQ_BIG_LQ ? 1 : 4;         // partial tiles of the small MFMA products (see the kernels)
    const size_t shmA = (size_t)(TILE_M * CATP + TILE_M * LDP + 2 * TILE_M * (Lq + 1) + 72 + npart * TILE_M * (32 * ((Lq + 31) / 32) + 1)) * sizeof(float);
    const size_t shmB = (size_t)(32 * ((Lq + 31) / 32) * LDP + TILE_M * LDP + TILE_M * (Lq + 1) + npart * TILE_M * (32 * ((Lq + 31) / 32) + 1)) * sizeof(float);
    const size_t shmC = (size_t)((Lq > CQ_BIG_LQ ? 1 : 2) * Lq * LDP + 2 * TILE_M * LDP + 2 * TILE_M * (Lq + 1) + 16 + Lq + TILE_M + 4 * D) * sizeof(float);
    // VIDX (a.vidx != nullptr, vsl_backward_shared): the reads of C go through the index, one scalar load per workgroup, as in the forward kernels
    auto go = [&](auto vx, const char* na, const char* nb, const char* nc) {
        constexpr bool VIDX = decltype(vx)::value;
        constexpr auto ka = k_cq_bwd_a<VIDX>, kb = k_cq_bwd_b<VIDX>, kc = k_cq_bwd_c<VIDX>;
        dynamic_lds_optin<ka>(shmA, na);
        dynamic_lds_optin<kb>(shmB, nb);
        dynamic_lds_optin<kc>(shmC, nc);
        VSL_LAUNCH(ka, dim3(ntile, B), dim3(256), shmA, s, a);
        { static int left = 2; if (stamps::enabled()) stamps::report("cq_bwd_a: load | gemm512 | Dc store | C load + c2q/q2c | product rule | dS_row + partials | sync | softmax bwd", 8, s, left); }
        VSL_LAUNCH(kb, dim3(ntile, B), dim3(256), shmB, s, a);
        VSL_LAUNCH(kc, dim3(ntile, B), dim3(256), shmC, s, a);
    };
    if (a.vidx) go(std::true_type{}, "k_cq_bwd_a<true>", "k_cq_bwd_b<true>", "k_cq_bwd_c<true>");
    else go(std::false_type{}, "k_cq_bwd_a", "k_cq_bwd_b", "k_cq_bwd_c");
}
// the per-sample tail (dQ, pooled-query path): nothing on the video side reads its outputs, so it runs on the query stream
void launch_cq_bwd_query(const CqBwdArgs& a0, int B, hipStream_t s) {
    CqBwdArgs a = a0;
    const int Lq = a.Lq;
    a.ntile = (a.T + TILE_M - 1) / TILE_M;
    const size_t shmD = (size_t)(Lq * LDP + 2 * Lq + 4 * D) * sizeof(float);
    dynamic_lds_optin<k_cq_bwd_d>(shmD, "k_cq_bwd_d");
    VSL_LAUNCH(k_cq_bwd_d, dim3(B), dim3(256), shmD, s, a);
}

}  // namespace vsl
