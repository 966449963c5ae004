// Embedding kernels of the VSLNet hot path (gfx950), forward and backward: word + character embedding, the Embedding linear at widths the split
// kernel does not tile, and the trainable word table.  Every kernel cites the reference lines it reproduces or differentiates (layers_t7.py unless
// noted); parameter gradients leave as per-chunk PARTIAL SLABS that k_reduce (kernels_params.hip) sums.
#include "common.hpp"
#include "launch.hpp"
#include "stamps.hpp"

namespace vsl {

// =========================================================================================================
// a3/a4  word + character embedding (:25-72) -> concatenated (Rq, 300 + 100) row, ready for the a5 linear.
//   One workgroup per EF_CHUNK = 8 query words.
//   word part : F.embedding over [pad; unk; glove] (:41) + dropout.
//   char CNN  : 4 x [Conv2d(50 -> c, (1,k)) + bias + ReLU -> max over char positions]; the arg-max position is saved
//               (int8) for the backward.  The 15000 conv weights are staged once per workgroup into LDS TRANSPOSED
//               ([ci*k + kk][channel], channel fastest: conflict-free for lanes that own consecutive channels); the
//               dropped-out char embeddings of the 8 words are staged transposed ([word][ci][position], zero padded) so
//               the sliding window of a channel is 3 vector LDS reads.  thread = (word, channel) items, 8 positions
//               at a time, no predicates in the inner loop.  Requires 4 <= Lc <= MAX_LC.
// =========================================================================================================
constexpr int EF_CHUNK = 8;
// LCM = compile-time bound of Lc (24 covers Charades / TACoS words; 40 the longest ActivityNet tokens): EF_PT = LCM + 4 padded
// positions per (word, ci) row (LCM + 3 taps, multiple of 4)
template <int LCM>
__global__ __launch_bounds__(512) void k_embed_fwd(const int64_t* __restrict__ word_ids, const int64_t* __restrict__ char_ids,
                                                   const float* __restrict__ pad_vec, const float* __restrict__ unk_vec,
                                                   const float* __restrict__ glove, const float* __restrict__ char_tab,
                                                   CharConvPtrs cc, const float* __restrict__ wimg, float* __restrict__ E,
                                                   int8_t* __restrict__ argpos, int Rq, int Lc, int word_dim, int char_dim,
                                                   int cb, Drop dw, Drop dc) {
    constexpr int EF_PT = LCM + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wt = smem;                                   // [cb][4 taps][100 channels], taps beyond a channel's width = 0
    float* CeT = Wt + cb * 400;                         // [EF_CHUNK][cb][EF_PT]
    __shared__ int cids[EF_CHUNK * LCM];
    const int tid = threadIdx.x, NT = blockDim.x;      // 512 threads: two waves per SIMD hide the LDS latency of the item loop
    const int EW = word_dim + 100;
    const int rbeg = blockIdx.x * EF_CHUNK, nw = min(EF_CHUNK, Rq - rbeg);
    STAMP(0);
    // ---- one block of `cb` input channels at a time (cb = char_dim up to 64: a single block; main_t7.py:24's char_dim 100 = two of 52):
    //      the LDS footprint is set by cb, not by char_dim, and the accumulators of a position tile run across the blocks
    auto stage_w = [&](int c0, int cbn) {
        // weights: straight vector copy of rows c0 .. c0 + cbn of the [ci][4 taps][100 channels] image k_pack built this step
        // (channel fastest: conflict-free for lanes that own consecutive channels; taps beyond a kernel width are 0)
        const float4* wsrc = reinterpret_cast<const float4*>(wimg + (size_t)c0 * 400);
        for (int e0 = 0; e0 < cbn * 100; e0 += 8 * NT) {
            float4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = e0 + tid + q * NT;
                v[q] = e < cbn * 100 ? wsrc[e] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) { const int e = e0 + tid + q * NT; if (e < cbn * 100) reinterpret_cast<float4*>(Wt)[e] = v[q]; }
        }
    };
    auto stage_ce = [&](int c0, int cbn) {
        // the transposed dropped-out embeddings (zero beyond Lc and beyond the chunk)
        for (int pr = tid; pr < EF_CHUNK * cbn; pr += NT) {              // pair (word, ci): one padded row of EF_PT positions
            const int wi = pr / cbn, cl = pr - wi * cbn, ci = c0 + cl;
            float* row = CeT + (wi * cb + cl) * EF_PT;
            float v[LCM];
#pragma unroll
            for (int pp = 0; pp < LCM; ++pp)                            // all gathers of the row issued together
                v[pp] = (wi < nw && pp < Lc) ? char_tab[(size_t)cids[wi * LCM + pp] * char_dim + ci] : 0.f;
#pragma unroll
            for (int pp = 0; pp < LCM; ++pp)
                row[pp] = (pp < Lc) ? v[pp] * drop_mul(dc, (uint32_t)(((rbeg + wi) * Lc + pp) * char_dim + ci)) : 0.f;
#pragma unroll
            for (int pp = LCM; pp < EF_PT; ++pp) row[pp] = 0.f;
        }
    };
    if (cb >= char_dim) stage_w(0, char_dim);       // single block: the weight copy overlaps the id / word-vector phase
    // ---- char ids and word vectors (independent of everything below)
    for (int e = tid; e < EF_CHUNK * LCM; e += NT) {
        const int wi = e / LCM, pp = e - wi * LCM;
        cids[e] = (wi < nw && pp < Lc) ? (int)char_ids[(size_t)(rbeg + wi) * Lc + pp] : 0;
    }
    for (int e = tid; e < nw * word_dim; e += NT) {
        const int wi = e / word_dim, c = e - wi * word_dim;
        const int r = rbeg + wi;
        const int64_t wid = word_ids[r];
        const float* src = wid == 0 ? pad_vec : (wid == 1 ? unk_vec : glove + (size_t)(wid - 2) * word_dim);
        E[(size_t)r * EW + c] = src[c] * drop_mul(dw, (uint32_t)(r * word_dim + c));
    }
    __syncthreads();
    STAMP(1);
    // ---- char CNN on the matrix cores: out[p][oc] = sum_{kk, ci} Ce[p + kk][ci] W[oc][ci][kk] is a (positions x 4*char_dim)
    //      x (4*char_dim x 100) product per word (taps beyond a channel's kernel width are zero in the image).  wave = word,
    //      16 positions per MFMA tile, 7 tiles of 16 channels share every A operand; bias + ReLU + max / arg-max over the
    //      positions (:58, 69-70) happen in the accumulator registers and two shuffles.
    {
        const int w = tid >> 6, lane = tid & 63, jl = lane & 15, g4 = lane >> 4;
        const bool single = cb >= char_dim;
        if (single) { stage_ce(0, char_dim); __syncthreads(); }
        STAMP(2);
        const float* ce = CeT + w * cb * EF_PT;
        float best[7], bias[7];
        int bestp[7], kw[7];
#pragma unroll
        for (int nt = 0; nt < 7; ++nt) {
            const int oc = 16 * nt + jl;
            best[nt] = -1.f; bestp[nt] = 0;
            kw[nt] = oc < 10 ? 1 : oc < 30 ? 2 : oc < 60 ? 3 : 4;
            bias[nt] = oc < 10 ? cc.b[0][oc] : oc < 30 ? cc.b[1][oc - 10] : oc < 60 ? cc.b[2][oc - 30] : oc < 100 ? cc.b[3][oc - 60] : 0.f;
        }
        for (int mt = 0; 16 * mt < Lc; ++mt) {
            f32x4 acc[7];
#pragma unroll
            for (int nt = 0; nt < 7; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int c0 = 0; c0 < char_dim; c0 += cb) {
                const int cbn = min(cb, char_dim - c0);
                if (!single) { __syncthreads(); stage_w(c0, cbn); stage_ce(c0, cbn); __syncthreads(); }     // (block-uniform: every wave takes the barriers)
                if (w < nw) {
                    const int ncg = (cbn + 3) >> 2;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        // operands of step cg + 1 are requested before the MFMAs of step cg (one-deep register pipeline)
                        float av, bv[7], an, bn[7];
                        auto ld = [&](int cg, float& a_, float (&b_)[7]) {
                            const int ci = 4 * cg + g4;
                            const bool okc = ci < cbn;
                            a_ = okc ? ce[ci * EF_PT + 16 * mt + jl + kk] : 0.f;
                            const float* wr = Wt + (ci * 4 + kk) * 100 + jl;
#pragma unroll
                            for (int nt = 0; nt < 7; ++nt)
                                if ((kk < 2) || (kk == 2 && nt >= 1) || (kk == 3 && nt >= 3))
                                    b_[nt] = (okc && 16 * nt + jl < 100) ? wr[16 * nt] : 0.f;
                        };
                        ld(0, av, bv);
                        for (int cg = 0; cg < ncg; ++cg) {
                            if (cg + 1 < ncg) ld(cg + 1, an, bn);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int nt = 0; nt < 7; ++nt) {
                                // channel tiles whose widest kernel is narrower than this tap hold only zeros: skipped
                                if ((kk < 2) || (kk == 2 && nt >= 1) || (kk == 3 && nt >= 3))
                                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nt], acc[nt], 0, 0, 0);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            av = an;
#pragma unroll
                            for (int nt = 0; nt < 7; ++nt) bv[nt] = bn[nt];
                        }
                    }
                }
            }
#pragma unroll
            for (int nt = 0; nt < 7; ++nt) {
                const int npos = Lc - kw[nt] + 1;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int pp = 16 * mt + 4 * g4 + rr;
                    const float v = fmaxf(acc[nt][rr] + bias[nt], 0.f);
                    if (pp < npos && v > best[nt]) { best[nt] = v; bestp[nt] = pp; }     // first maximum wins
                }
            }
        }
        if (w < nw) {
            const int r = rbeg + w;
#pragma unroll
            for (int nt = 0; nt < 7; ++nt) {
                float bv = best[nt];
                int bp = bestp[nt];
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {               // combine the 4 position groups, lowest position on ties
                    const float ov = __shfl_xor(bv, o);
                    const int op = __shfl_xor(bp, o);
                    if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; }
                }
                const int oc = 16 * nt + jl;
                if (g4 == 0 && oc < 100) {
                    E[(size_t)r * EW + word_dim + oc] = bv;
                    if (argpos) argpos[(size_t)r * 100 + oc] = (int8_t)bp;      // (null in inference mode)
                }
            }
        }
    }
    STAMP(3);
}
template <int LCM> static void embed_fwd_go(const EmbedFwdArgs& a, int cb, const char* name, hipStream_t s) {
    const size_t shm = (size_t)(cb * 400 + EF_CHUNK * cb * (LCM + 4) + 32) * sizeof(float);   // + slack: invalid positions over-read
    dynamic_lds_optin<k_embed_fwd<LCM>>(shm, name);
    VSL_LAUNCH(k_embed_fwd<LCM>, dim3((a.Rq + EF_CHUNK - 1) / EF_CHUNK), dim3(512), shm, s, a.word_ids, a.char_ids, a.pad_vec, a.unk_vec, a.glove, a.char_tab, a.cc,
               a.wimg, a.E, a.argpos, a.Rq, a.Lc, a.word_dim, a.char_dim, cb, a.dw, a.dc);
}
void launch_embed_fwd(const EmbedFwdArgs& a, hipStream_t s) {
    const int char_dim = a.char_dim, lcm = a.Lc <= 24 ? 24 : MAX_LC;
    // input-channel block: as many channels as fit the 160 KB of LDS beside the word rows (64 with the short-token instantiation, 52 with the
    // long one); wider character embeddings run in equal blocks (multiples of 4) with the accumulators carried across them
    const int cb_max = lcm == 24 ? 64 : 52;
    const int nblk = (char_dim + cb_max - 1) / cb_max;
    const int cb = nblk == 1 ? char_dim : (((char_dim + nblk - 1) / nblk) + 3) & ~3;
    if (lcm == 24) embed_fwd_go<24>(a, cb, "k_embed_fwd<24>", s); else embed_fwd_go<MAX_LC>(a, cb, "k_embed_fwd<40>", s);
    static int left = 2;
    if (stamps::enabled()) stamps::report("embed_fwd: ids+words | weights+CeT | items", 4, s, left);
}

// =========================================================================================================
// generic row-tile linear  Y = A W^T + b  (Conv1D k=1, :12-22) for an (R, K) row-major A, K % 8 == 0.
// The a5 Embedding.linear at a width the split kernel's 16-wide K steps do not tile (launch_linear_fwd3 otherwise).  A is staged through LDS in
// 128-wide chunks.
// =========================================================================================================
__global__ __launch_bounds__(256) void k_linear_fwd(const float* __restrict__ A, const float* __restrict__ Wpack,
                                                    const float* __restrict__ bias, float* __restrict__ Y, int R, int K) {
    __shared__ __attribute__((aligned(16))) float As[TILE_M * LDP];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * TILE_M;
    f32x16 acc[1];
    zero_acc(acc);
    for (int k0 = 0; k0 < K; k0 += 128) {
        const int kc = min(128, K - k0);
        for (int e = tid; e < TILE_M * 32; e += 256) {
            const int rr = e >> 5, c = (e & 31) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + rr < R && c < kc) v = *reinterpret_cast<const float4*>(A + (size_t)(r0 + rr) * K + k0 + c);
            *reinterpret_cast<float4*>(&As[rr * LDP + c]) = v;
        }
        const float* wp = Wpack + (size_t)(k0 / 8) * D * 8;
        BFrag<1, 16> bf;
        bfrag_load(bf, wp, D, 32 * w, 0, 0, kc >> 3);
        __syncthreads();
        gemm32p<1, 16>(As, LDP, kc, wp, D, 32 * w, 0, acc, bf);
        __syncthreads();
    }
    const int col = 32 * w + (lane & 31);
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gr = r0 + acc_row(r, lane);
        if (gr < R) Y[(size_t)gr * D + col] = acc[0][r] + bv;
    }
}
void launch_linear_fwd(const float* A, const float* Wpack, const float* bias, float* Y, int R, int K, hipStream_t s) {
    VSL_LAUNCH(k_linear_fwd, dim3((R + TILE_M - 1) / TILE_M), dim3(256), 0, s, A, Wpack, bias, Y, R, K);
}

// =========================================================================================================
// a3 / a4 backward: unk_vec gradient, char-CNN weights / biases, char table (padding_idx = 0 gets none).
//   One workgroup of 8 waves per `chunk` query words (embed_bwd_chunk: as many as keep the grid inside one round of the 256 CUs);
//   the rows (word, position) of the chunk are packed densely.  Nothing here is sized by char_dim beyond an LDS row stride of 64
//   or 128 floats (char_dim <= 128; main_t7.py:24 prescribes 100 for ActivityNet).  After two shared staging phases the waves split
//   into two roles that never meet again:
//   waves 4-7 (i)   dW[oc][ci][kk] += g[oc] * Ce[pos[oc] + kk][ci]   thread = 25 fixed (oc, ci) pairs, 4 tap accumulators each: one
//         {pos, g} lookup per pair and word (one 8-byte LDS broadcast), shared by the taps.  Exact fp32 FMAs.
//   waves 0-3 (ii)  dCe[row][ci] = sum_k G[row][k] W[k][ci] over the k = (tap, channel) pairs of the four convs, where G has ONE
//         non-zero per (word, k): the arg-max position of the channel shifted by the tap.  The product runs on the matrix cores (wave
//         = 16 input channels, 76 MFMAs of 16x16x4 per 16-row tile) and G is never materialised: a lane builds its A operand from the
//         {pos, g} pair of (word, channel) -- g * (pos + tap == position) -- so there is no scatter, no clear and no barrier between
//         tiles.  k runs tap-major over aligned channel ranges (tap 0: channels 0..99, tap 1: 8..99, tap 2: 28..99, tap 3: 60..99; the
//         channels below a conv's first one carry zero weights), which makes (tap, channel) of an unrolled step a compile-time
//         constant plus lane >> 4.  The B operands (76 values per lane) come from an image k_pack lays out in lane order.
//         (iii) table[cid][ci] += dCe[row][ci] for the character of every row: ALSO a product on the matrix cores,
//         onehot[cid][row] x dCe[row][ci] (the one-hot operand is exact, the accumulation order is fixed: deterministic, no atomics,
//         no serial per-character loop, no LDS accumulator).  The wave that produced a channel tile of dCe consumes it: no barrier.
//   (Round 2 scattered G into LDS one word at a time -- two barriers, a clear and a 10-step serial table update per word: phases (ii)
//   + (iii) were 53 k of the kernel's 91 k cycles, and (i) ran before them on the same four waves.)
// =========================================================================================================
constexpr int EB_NP = 25;                     // (100 channels x 64 lanes) / 256 threads of the dW role
constexpr int EB_NQ = 76;                     // k-steps of 4 (tap, channel) pairs: 25 + 23 + 18 + 10
constexpr int EB_GS = 305;                    // LDS row stride of G (odd: conflict-free column reads)
__host__ __device__ constexpr int eb_tap(int q) { return q < 25 ? 0 : q < 48 ? 1 : q < 66 ? 2 : 3; }
__host__ __device__ constexpr int eb_oc0(int q) { return q < 25 ? 4 * q : q < 48 ? 8 + 4 * (q - 25) : q < 66 ? 28 + 4 * (q - 48) : 60 + 4 * (q - 66); }
__global__ __launch_bounds__(512) void k_embed_bwd(const float* __restrict__ dE, const int64_t* __restrict__ word_ids,
                                                   const int64_t* __restrict__ char_ids, const float* __restrict__ E,
                                                   const int8_t* __restrict__ argpos, const float* __restrict__ char_tab,
                                                   const float* __restrict__ wimg_b, float* __restrict__ p_cw, float* __restrict__ p_cb,
                                                   float* __restrict__ p_tab, float* __restrict__ p_unk, int Rq, int Lc,
                                                   int word_dim, int char_dim, int char_size, int cdp, int chunk, Drop dw, Drop dc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wtot = char_dim * 300;          // 10*1 + 20*2 + 30*3 + 40*4 = 300 taps per input channel
    const int ds = cdp + 16;                  // row stride of dce: the 4 k-rows of a B operand land in disjoint banks
    float* Ce = smem;                         // [chunk * Lc + 4][cdp] dropped char embeddings (+ zero rows)
    float* dce = Ce + (chunk * Lc + 4) * cdp;                     // [chunk * Lc][ds] char-embedding gradients
    int2* gp = reinterpret_cast<int2*>(dce + chunk * Lc * ds);    // [chunk][128] {arg-max position, gradient bits} (0 where inactive)
    int* cids = reinterpret_cast<int*>(gp + chunk * 128);         // [chunk * Lc + 4] character of every row
    float* Gm = reinterpret_cast<float*>(cids + ((chunk * Lc + 4 + 3) & ~3));   // [16 * ceil(rows / 16)][EB_GS] the tap matrix G (<= 300 non-zeros per word)
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, jl = lane & 15, g4 = lane >> 4;
    const int EW = word_dim + 100;
    const int rbeg = blockIdx.x * chunk, nw = min(chunk, Rq - rbeg);
    const int nrow = nw * Lc;
    const int nct = (char_dim + 15) >> 4;
    STAMP(0);
    // B operand of every MFMA of phase (ii): row-independent -> registers; the first channel tile of the wave is requested before
    // anything else so its latency hides behind the staging phases
    float wreg[EB_NQ];
    auto load_w = [&](int ct) {
        const float* src = wimg_b + (size_t)ct * EB_NQ * 64 + lane;
#pragma unroll
        for (int q = 0; q < EB_NQ; ++q) wreg[q] = src[q * 64];
    };
    if (w < 4 && w < nct) load_w(w);
    // ---- staging phase 1: G cleared, per-word metadata with all loads issued together
    {
        const int n4 = (((chunk * Lc + 15) >> 4) * 16 * EB_GS + 3) >> 2;
        for (int e = tid; e < n4; e += 512) reinterpret_cast<float4*>(Gm)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int e = tid; e < chunk * Lc + 4; e += 512) cids[e] = e < nrow ? (int)char_ids[(size_t)rbeg * Lc + e] : 0;
    for (int e = tid; e < chunk * 128; e += 512) {
        const int wi = e >> 7, oc = e & 127;
        float g = 0.f;
        int ps = 0;
        if (wi < nw && oc < 100) {
            const size_t o = (size_t)(rbeg + wi) * EW + word_dim + oc;
            g = E[o] > 0.f ? dE[o] : 0.f;                                  // relu + max: grad only to an active arg-max
            ps = argpos[(size_t)(rbeg + wi) * 100 + oc];
        }
        gp[e] = make_int2(ps, __float_as_int(g));
    }
    float uacc = 0.f;
    if (p_unk && tid < word_dim) {
        // unk_vec row of the [pad; unk; glove] table (:41): every row load of the chunk issued unconditionally, then masked
        float u[EMB_CHUNK_MAX];
#pragma unroll
        for (int wi = 0; wi < EMB_CHUNK_MAX; ++wi) u[wi] = wi < nw ? dE[(size_t)(rbeg + wi) * EW + tid] : 0.f;
#pragma unroll
        for (int wi = 0; wi < EMB_CHUNK_MAX; ++wi)
            if (wi < nw && word_ids[rbeg + wi] == 1) uacc += u[wi] * drop_mul(dw, (uint32_t)((rbeg + wi) * word_dim + tid));
    }
    __syncthreads();
    STAMP(1);
    // ---- staging phase 2: scatter G (one entry per (word, tap): row = word * Lc + pos[oc] + kk, column = the tap-major k of (kk, oc));
    //      gather the dropped-out char embeddings of every row of the chunk (+ 4 zero rows: taps past the last row)
    for (int e = tid; e < nw * 300; e += 512) {
        const int wi = e / 300, k = e - wi * 300;
        // taps in conv order: 10 x 1, 20 x 2, 30 x 3, 40 x 4
        int oc, kk;
        if (k < 10) { oc = k; kk = 0; }
        else if (k < 50) { oc = 10 + ((k - 10) >> 1); kk = (k - 10) & 1; }
        else if (k < 140) { oc = 30 + (k - 50) / 3; kk = (k - 50) - 3 * (oc - 30); }
        else { oc = 60 + ((k - 140) >> 2); kk = (k - 140) & 3; }
        const int2 pg = gp[wi * 128 + oc];
        const int col = kk == 0 ? oc : kk == 1 ? 100 + oc - 8 : kk == 2 ? 192 + oc - 28 : 264 + oc - 60;
        Gm[(wi * Lc + pg.x + kk) * EB_GS + col] = __int_as_float(pg.y);
    }
    {
        const int sh = cdp == 64 ? 6 : 7;
        for (int e = tid; e < (chunk * Lc + 4) * cdp; e += 512) {
            const int row = e >> sh, ci = e & (cdp - 1);
            float v = 0.f;
            if (row < nrow && ci < char_dim)
                v = char_tab[(size_t)cids[row] * char_dim + ci] * drop_mul(dc, (uint32_t)((rbeg * Lc + row) * char_dim + ci));
            Ce[e] = v;
        }
    }
    __syncthreads();
    STAMP(2);
    if (w >= 4) {
        // ---- (i) conv weight / bias gradients: pair q of this thread = (oc = ((tid >> 6) - 4) + 4 q, ci = cih + (tid & 63))
        const int s0 = 10 * char_dim, s1 = 20 * char_dim * 2, s2 = 30 * char_dim * 3;
        const int t = tid - 256;
        float bacc = 0.f;
        for (int cih = 0; cih < char_dim; cih += 64) {
            float wacc[EB_NP][4];
#pragma unroll
            for (int q = 0; q < EB_NP; ++q) { wacc[q][0] = 0.f; wacc[q][1] = 0.f; wacc[q][2] = 0.f; wacc[q][3] = 0.f; }
            const int ci = cih + lane, ocb = w - 4;
            for (int wi = 0; wi < nw; ++wi) {
                const int2* g = gp + wi * 128;
                const float* ce = Ce + wi * Lc * cdp + ci;
                if (cih == 0 && t < 100) bacc += __int_as_float(g[t].y);
#pragma unroll
                for (int q = 0; q < EB_NP; ++q) {
                    const int2 pg = g[ocb + 4 * q];
                    const float gv = __int_as_float(pg.y);
                    const float* row = ce + pg.x * cdp;       // taps beyond the kernel width read later rows / zero rows: unused
                    wacc[q][0] += gv * row[0];
                    wacc[q][1] += gv * row[cdp];
                    wacc[q][2] += gv * row[2 * cdp];
                    wacc[q][3] += gv * row[3 * cdp];
                }
            }
            if (ci < char_dim) {
                float* dst = p_cw + (size_t)blockIdx.x * wtot;
#pragma unroll
                for (int q = 0; q < EB_NP; ++q) {
                    const int oc = ocb + 4 * q;               // slab offsets are multiples of 4 floats: the vector stores are aligned
                    if (oc < 10) dst[oc * char_dim + ci] = wacc[q][0];
                    else if (oc < 30) *reinterpret_cast<float2*>(dst + s0 + ((oc - 10) * char_dim + ci) * 2) = make_float2(wacc[q][0], wacc[q][1]);
                    else if (oc < 60) {
                        float* d3 = dst + s0 + s1 + ((oc - 30) * char_dim + ci) * 3;
                        d3[0] = wacc[q][0]; d3[1] = wacc[q][1]; d3[2] = wacc[q][2];
                    } else
                        *reinterpret_cast<float4*>(dst + s0 + s1 + s2 + ((oc - 60) * char_dim + ci) * 4) =
                            make_float4(wacc[q][0], wacc[q][1], wacc[q][2], wacc[q][3]);
                }
            }
        }
        if (t < 100) p_cb[(size_t)blockIdx.x * 100 + t] = bacc;
    } else {
        // ---- (ii) + (iii)
        const int nrt = (nrow + 15) >> 4, nmc = (char_size + 15) >> 4;
        for (int ct = w; ct < nct; ct += 4) {
            const int ci = 16 * ct + jl;
            if (ct != w) load_w(ct);
            for (int rt = 0; rt < nrt; ++rt) {
                const float* grow = Gm + (16 * rt + jl) * EB_GS + g4;     // A operand: row = (word, position), k-slot = lane >> 4
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < EB_NQ; q += 2) {
                    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(grow[4 * q], wreg[q], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(grow[4 * q + 4], wreg[q + 1], a1, 0, 0, 0);
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int ro = 16 * rt + 4 * g4 + rr;
                    if (ro < nrow)
                        dce[ro * ds + ci] = ci < char_dim ? (a0[rr] + a1[rr]) * drop_mul(dc, (uint32_t)((rbeg * Lc + ro) * char_dim + ci)) : 0.f;
                }
            }
            STAMP(3);
            // (iii): the rows of this channel tile were written by this very wave (LDS is in order within a wave)
            for (int mc0 = 0; mc0 < nmc; mc0 += 4) {
                f32x4 acc[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int r0 = 0; r0 < nrow; r0 += 16) {
                    int cv[4];
                    float bv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int row = r0 + 4 * u + g4;
                        const bool ok = row < nrow;
                        cv[u] = ok ? cids[row] : -1;
                        bv[u] = ok ? dce[row * ds + ci] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            if (mc0 + m < nmc)
                                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[u] == 16 * (mc0 + m) + jl ? 1.f : 0.f, bv[u], acc[m], 0, 0, 0);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int co = 16 * (mc0 + m) + 4 * g4 + rr;
                        if (co < char_size && ci < char_dim)
                            p_tab[(size_t)blockIdx.x * char_size * char_dim + co * char_dim + ci] = co != 0 ? acc[m][rr] : 0.f;   // padding_idx = 0 (:51)
                    }
            }
        }
        STAMP(4);
    }
    if (p_unk && tid < word_dim) p_unk[(size_t)blockIdx.x * word_dim + tid] = uacc;
}
// words per workgroup: the smallest chunk whose grid fits one round of the 256 CUs, at least 4 (slab traffic), at most 8 and at most
// 80 (char_dim <= 64) / 48 rows (the LDS footprint: 145 / 113 KB at the bound)
int embed_bwd_chunk(int Rq, int Lc, int char_dim) {
    int c = (Rq + 255) / 256;
    c = c < 4 ? 4 : c > EMB_CHUNK_MAX ? EMB_CHUNK_MAX : c;
    const int rmax = (char_dim <= 64 ? 80 : 48) / Lc;
    return c > rmax ? (rmax < 1 ? 1 : rmax) : c;
}
void launch_embed_bwd(const EmbedBwdArgs& a, hipStream_t s) {
    const int Rq = a.Rq, Lc = a.Lc, cdp = a.char_dim <= 64 ? 64 : 128, chunk = embed_bwd_chunk(Rq, Lc, a.char_dim);
    const size_t shm = (size_t)((chunk * Lc + 4) * cdp + chunk * Lc * (cdp + 16) + chunk * 256 + ((chunk * Lc + 4 + 3) & ~3) +
                                ((chunk * Lc + 15) / 16) * 16 * EB_GS + 4) * sizeof(float);
    dynamic_lds_optin<k_embed_bwd>(shm, "k_embed_bwd");
    VSL_LAUNCH(k_embed_bwd, dim3((Rq + chunk - 1) / chunk), dim3(512), shm, s, a.dE, a.word_ids, a.char_ids, a.E, a.argpos, a.char_tab, a.wimg_b, a.p_cw, a.p_cb,
               a.p_tab, a.p_unk, Rq, Lc, a.word_dim, a.char_dim, a.char_size, cdp, chunk, a.dw, a.dc);
    static int left = 2;
    if (stamps::enabled()) stamps::report("embed_bwd: metadata | gather | dCe | table (waves 0-3)", 5, s, left);
}

// =========================================================================================================
// a3 backward of the TRAINABLE word table (WordEmbedding(word_vectors=None), layers_t7.py:36: nn.Embedding(word_size, word_dim,
// padding_idx=0)): gtab[wid] = sum over the occurrences of wid in the batch of dE[r][:word_dim] * dropout mask, rows that do not occur
// and row 0 are zero.  Dense gradient, as torch.optim.AdamW sees it.  One workgroup per occurrence r: it owns the table row only if no
// earlier row holds the same word, and then adds the occurrences in ascending r -- a fixed order: deterministic without atomics.  The
// table region is cleared by k_zero4 first (the reduction kernel does not cover it).
// k_word_table_bwd_acc (vsl_backward_accumulate): nothing is cleared; the owner of a row stores prev + acc (one fp32 add behind the same sum), and a row no word
// of this batch touches keeps its value.
// =========================================================================================================
__global__ __launch_bounds__(256) void k_zero4(float4* __restrict__ dst, int64_t n4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) dst[e] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ __launch_bounds__(128) void k_word_table_bwd(const float* __restrict__ dE, const int64_t* __restrict__ word_ids,
                                                        float* __restrict__ gtab, int Rq, int word_dim, Drop dw) {
    const int r = blockIdx.x, tid = threadIdx.x, EW = word_dim + 100;
    const int64_t wid = word_ids[r];
    if (wid == 0) return;                              // padding_idx = 0
    __shared__ int seen;
    if (tid == 0) seen = 0;
    __syncthreads();
    bool mine = false;
    for (int q = tid; q < r; q += 128) mine |= word_ids[q] == wid;
    if (mine) seen = 1;
    __syncthreads();
    if (seen) return;                                  // an earlier occurrence owns this table row
    float acc[4] = {0.f, 0.f, 0.f, 0.f};              // word_dim <= 512
    for (int q = r; q < Rq; ++q)
        if (word_ids[q] == wid) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tid + 128 * j;
                if (c < word_dim) acc[j] += dE[(size_t)q * EW + c] * drop_mul(dw, (uint32_t)(q * word_dim + c));
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + 128 * j;
        if (c < word_dim) gtab[(size_t)wid * word_dim + c] = acc[j];
    }
}
// the accumulating form.  A kernel of its own, not an instantiation of a shared body: with the body in a template the compiler lays the plain
// kernel's exits out differently, and that kernel keeps its machine code (profiles/accum_kernel_resources.txt)
__global__ __launch_bounds__(128) void k_word_table_bwd_acc(const float* __restrict__ dE, const int64_t* __restrict__ word_ids,
                                                            float* __restrict__ gtab, int Rq, int word_dim, Drop dw) {
    const int r = blockIdx.x, tid = threadIdx.x, EW = word_dim + 100;
    const int64_t wid = word_ids[r];
    if (wid == 0) return;                              // padding_idx = 0
    __shared__ int seen;
    if (tid == 0) seen = 0;
    __syncthreads();
    bool mine = false;
    for (int q = tid; q < r; q += 128) mine |= word_ids[q] == wid;
    if (mine) seen = 1;
    __syncthreads();
    if (seen) return;                                  // an earlier occurrence owns this table row
    float acc[4] = {0.f, 0.f, 0.f, 0.f};              // word_dim <= 512
    for (int q = r; q < Rq; ++q)
        if (word_ids[q] == wid) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tid + 128 * j;
                if (c < word_dim) acc[j] += dE[(size_t)q * EW + c] * drop_mul(dw, (uint32_t)(q * word_dim + c));
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + 128 * j;
        if (c < word_dim) gtab[(size_t)wid * word_dim + c] = gtab[(size_t)wid * word_dim + c] + acc[j];
    }
}
void launch_word_table_bwd(const float* dE, const int64_t* word_ids, float* gtab, int Rq, int word_size, int word_dim, Drop dw, bool accumulate, hipStream_t s) {
    if (accumulate) {
        VSL_LAUNCH(k_word_table_bwd_acc, dim3(Rq), dim3(128), 0, s, dE, word_ids, gtab, Rq, word_dim, dw);
        return;
    }
    const int64_t n4 = (int64_t)word_size * word_dim / 4;       // (the flat bucket keeps every parameter 4-float aligned; word_dim % 4 == 0)
    const int zb = (int)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
    VSL_LAUNCH(k_zero4, dim3(zb), dim3(256), 0, s, reinterpret_cast<float4*>(gtab), n4);
    VSL_LAUNCH(k_word_table_bwd, dim3(Rq), dim3(128), 0, s, dE, word_ids, gtab, Rq, word_dim, dw);
}

}  // namespace vsl
