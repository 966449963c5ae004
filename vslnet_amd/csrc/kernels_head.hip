// Head kernels of the VSLNet hot path (gfx950), forward and backward: the attention-output block of an encoder application as a launch of its own,
// the span heads, the losses with their gradient seeds, and extract_index.  The loss lives beside the heads because k_head_bwd computes its inline
// seeds through the same loss_sample_lse.  Every kernel cites the reference lines it reproduces or differentiates (layers_t7.py unless noted);
// parameter gradients leave as per-tile PARTIAL SLABS that k_reduce (kernels_params.hip) sums.
#include "common.hpp"
#include "launch.hpp"
#include "tile_bodies.hpp"

namespace vsl {

// =========================================================================================================
// a13 + a16 losses (layers_t7.py:291-299, 365-369) and their seeds d(total)/d(logits), d(total)/d(h_score)
//   total = w_loc * (CE(start) + CE(end)) + w_hl * highlight      (main_t7.py:105-107 uses 1, 5)
//   scratch layout (floats): [0,B) lse_s | [B,2B) lse_e | [2B,3B) ce | [3B,4B) hl numerator | [4B,5B) mask sum
// =========================================================================================================
// block_reduce, loss_sample_lse and loss_store: tile_bodies.hpp, beside the per-element terms and seeds (kernels_group_loss.hip builds the grouped
// loss from the same functions)
__global__ __launch_bounds__(256) void k_loss_a(const float* __restrict__ sl, const float* __restrict__ el,
                                                const float* __restrict__ h, const int64_t* __restrict__ s_lab,
                                                const int64_t* __restrict__ e_lab, const int64_t* __restrict__ h_lab,
                                                const float* __restrict__ vmask, int B, int T, float* __restrict__ scratch) {
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* s = sl + (size_t)b * T;
    const float* e = el + (size_t)b * T;
    const float lses = loss_sample_lse(s, T, red), lsee = loss_sample_lse(e, T, red);
    float num = 0.f, den = 0.f;
    for (int t = tid; t < T; t += 256) {
        const size_t i = (size_t)b * T + t;
        const float m = vmask[i];
        num += loss_hl_term(h[i], (float)h_lab[i], m);
        den += m;
    }
    num = block_reduce(num, red, false);
    den = block_reduce(den, red, false);
    if (tid == 0) {
        scratch[b] = lses;
        scratch[B + b] = lsee;
        scratch[2 * B + b] = (lses - s[s_lab[b]]) + (lsee - e[e_lab[b]]);
        scratch[3 * B + b] = num;
        scratch[4 * B + b] = den;
    }
}
__global__ __launch_bounds__(256) void k_loss_b(int B, float inv_batch, float mask_sum_override, float w_loc, float w_hl,
                                                const float* __restrict__ scratch, float* __restrict__ losses) {
    __shared__ float red[8];
    float ce = 0.f, num = 0.f, den = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) { ce += scratch[2 * B + b]; num += scratch[3 * B + b]; den += scratch[4 * B + b]; }
    ce = block_reduce(ce, red, false);
    num = block_reduce(num, red, false);
    den = block_reduce(den, red, false);
    if (threadIdx.x == 0) loss_store(losses, ce, num, mask_sum_override > 0.f ? mask_sum_override : den, inv_batch, w_loc, w_hl);
}
// gradient seeds + (block (0,0)) the loss values: every block re-reduces the B per-sample partials itself (a few hundred
// floats, L2-resident), which saves the single-block kernel between k_loss_a and this one on the critical path
__global__ __launch_bounds__(256) void k_loss_c(const float* __restrict__ sl, const float* __restrict__ el,
                                                const float* __restrict__ h, const int64_t* __restrict__ s_lab,
                                                const int64_t* __restrict__ e_lab, const int64_t* __restrict__ h_lab,
                                                const float* __restrict__ vmask, int B, int T, float inv_batch,
                                                float mask_sum_override, float w_loc, float w_hl,
                                                const float* __restrict__ scratch, float* __restrict__ losses,
                                                float* __restrict__ d_sl, float* __restrict__ d_el, float* __restrict__ d_h) {
    __shared__ float red[8];
    float ce = 0.f, num = 0.f, den = 0.f;
    for (int bb = threadIdx.x; bb < B; bb += 256) { ce += scratch[2 * B + bb]; num += scratch[3 * B + bb]; den += scratch[4 * B + bb]; }
    ce = block_reduce(ce, red, false);
    num = block_reduce(num, red, false);
    den = block_reduce(den, red, false);
    const float dsum = mask_sum_override > 0.f ? mask_sum_override : den;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) loss_store(losses, ce, num, dsum, inv_batch, w_loc, w_hl);
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t i = (size_t)b * T + t;
    const float cs = w_loc * inv_batch;
    d_sl[i] = loss_ce_seed(sl[i], scratch[b], t, (int)s_lab[b], cs);
    d_el[i] = loss_ce_seed(el[i], scratch[B + b], t, (int)e_lab[b], cs);
    d_h[i] = loss_hl_seed(h[i], (float)h_lab[i], vmask[i], w_hl, dsum);
}
// One launch when the caller supplies the global mask sum (the data-parallel path and bench.py do): the sample's workgroup writes its
// gradient seeds itself -- they need nothing from other samples then -- and the LAST workgroup to arrive (agent-scope counter) adds the
// per-sample partials in index order, so the loss values do not depend on which one that is.  Saves k_loss_c on the critical chain.
__global__ __launch_bounds__(256) void k_loss_fused(const float* __restrict__ sl, const float* __restrict__ el,
                                                    const float* __restrict__ h, const int64_t* __restrict__ s_lab,
                                                    const int64_t* __restrict__ e_lab, const int64_t* __restrict__ h_lab,
                                                    const float* __restrict__ vmask, int B, int T, float inv_batch, float mask_sum,
                                                    float w_loc, float w_hl, float* __restrict__ scratch, float* __restrict__ losses,
                                                    float* __restrict__ d_sl, float* __restrict__ d_el, float* __restrict__ d_h,
                                                    unsigned* __restrict__ counter) {
    __shared__ float red[8];
    __shared__ unsigned last;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* s = sl + (size_t)b * T;
    const float* e = el + (size_t)b * T;
    const float lses = loss_sample_lse(s, T, red), lsee = loss_sample_lse(e, T, red);
    float num = 0.f;
    for (int t = tid; t < T; t += 256) {
        const size_t i = (size_t)b * T + t;
        num += loss_hl_term(h[i], (float)h_lab[i], vmask[i]);
    }
    num = block_reduce(num, red, false);
    const float cs = w_loc * inv_batch;
    const int sb = (int)s_lab[b], eb = (int)e_lab[b];
    for (int t = tid; t < T; t += 256) {
        const size_t i = (size_t)b * T + t;
        d_sl[i] = loss_ce_seed(s[t], lses, t, sb, cs);
        d_el[i] = loss_ce_seed(e[t], lsee, t, eb, cs);
        d_h[i] = loss_hl_seed(h[i], (float)h_lab[i], vmask[i], w_hl, mask_sum);
    }
    if (tid == 0) {
        // the two partials go out WRITE-THROUGH (sc1 stores) and are drained before the arrival is counted; the last arriver reads them with
        // sc1 loads.  No fence on either side: __threadfence() is an L2 write-back + invalidate on this part, ~3.5 us -- twice on the chain
        // of a kernel that has 4 us of work (MI355X_MICROARCH.md, visibility; the protocol of the rnn head's granules)
        __hip_atomic_store(scratch + 2 * B + b, (lses - s[sb]) + (lsee - e[eb]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(scratch + 3 * B + b, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(B - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    float ce = 0.f, nm = 0.f;
    for (int bb = tid; bb < B; bb += 256) {                                 // L2 reads: another CU wrote these
        ce += __hip_atomic_load(scratch + 2 * B + bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nm += __hip_atomic_load(scratch + 3 * B + bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ce = block_reduce(ce, red, false);
    nm = block_reduce(nm, red, false);
    if (tid == 0) {
        loss_store(losses, ce, nm, mask_sum, inv_batch, w_loc, w_hl);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // ready for the next call (stream order)
    }
}
void launch_loss(const LossArgs& a, hipStream_t s) {
    const int B = a.B, T = a.T;
    if (a.counter && a.d_sl && a.mask_sum > 0.f) {     // the caller supplies the global mask sum (data-parallel path): one launch
        VSL_LAUNCH(k_loss_fused, dim3(B), dim3(256), 0, s, a.sl, a.el, a.h, a.s_lab, a.e_lab, a.h_lab, a.vmask, B, T, a.inv_batch, a.mask_sum,
                   a.w_loc, a.w_hl, a.scratch, a.losses, a.d_sl, a.d_el, a.d_h, a.counter);
        return;
    }
    VSL_LAUNCH(k_loss_a, dim3(B), dim3(256), 0, s, a.sl, a.el, a.h, a.s_lab, a.e_lab, a.h_lab, a.vmask, B, T, a.scratch);
    if (a.d_sl)
        VSL_LAUNCH(k_loss_c, dim3((T + 255) / 256, B), dim3(256), 0, s, a.sl, a.el, a.h, a.s_lab, a.e_lab, a.h_lab, a.vmask, B, T,
                   a.inv_batch, a.mask_sum, a.w_loc, a.w_hl, a.scratch, a.losses, a.d_sl, a.d_el, a.d_h);
    else
        VSL_LAUNCH(k_loss_b, dim3(1), dim3(256), 0, s, B, a.inv_batch, a.mask_sum, a.w_loc, a.w_hl, a.scratch, a.losses);
}

// a17 extract_index (:355-363): argmax over the upper-triangular outer product of the two softmaxes, computed as
//   start = argmax_i ps[i] * max_{j>=i} pe[j],  end = argmax_j pe[j] * max_{i<=j} ps[i]   (no (B,T,T) tensor)
__global__ __launch_bounds__(256) void k_extract_index(const float* __restrict__ sl, const float* __restrict__ el,
                                                       int64_t* __restrict__ si, int64_t* __restrict__ ei, int T) {
    extern __shared__ float sm[];
    float* ps = sm;
    float* pe = sm + T;
    float* red = pe + T;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* s = sl + (size_t)b * T;
    const float* e = el + (size_t)b * T;
    float ms = -3.0e38f, me = -3.0e38f;
    for (int t = tid; t < T; t += 256) { ms = fmaxf(ms, s[t]); me = fmaxf(me, e[t]); }
    ms = block_reduce(ms, red, true);
    me = block_reduce(me, red, true);
    float ss = 0.f, se = 0.f;
    for (int t = tid; t < T; t += 256) {
        const float a = expf(s[t] - ms), c = expf(e[t] - me);
        ps[t] = a; pe[t] = c; ss += a; se += c;
    }
    ss = block_reduce(ss, red, false);
    se = block_reduce(se, red, false);
    for (int t = tid; t < T; t += 256) { ps[t] = ps[t] / ss; pe[t] = pe[t] / se; }
    __syncthreads();
    if (tid == 0) {          // start: scan from the right keeping the suffix max of pe
        float suf = 0.f, best = -1.f;
        int bi = 0;
        for (int i = T - 1; i >= 0; --i) {
            suf = fmaxf(suf, pe[i]);
            const float v = ps[i] * suf;
            if (v >= best) { best = v; bi = i; }       // >= while scanning right-to-left keeps the FIRST maximal index
        }
        si[b] = bi;
    } else if (tid == 64) {  // end: scan from the left keeping the prefix max of ps
        float pre = 0.f, best = -1.f;
        int bi = 0;
        for (int j = 0; j < T; ++j) {
            pre = fmaxf(pre, ps[j]);
            const float v = pe[j] * pre;
            if (v > best) { best = v; bi = j; }
        }
        ei[b] = bi;
    }
}
void launch_extract_index(const float* sl, const float* el, int64_t* si, int64_t* ei, int B, int T, hipStream_t s) {
    VSL_LAUNCH(k_extract_index, dim3(B), dim3(256), (size_t)(2 * T + 8) * sizeof(float), s, sl, el, si, ei, T);
}

// =========================================================================================================
// a8 (second half)  r = drop(att) + x ; y = drop( drop(LN2(r)) Wo^T + bo ) + r      (:183-190)
// =========================================================================================================
__global__ __launch_bounds__(256) void k_attn_out_fwd(const float* __restrict__ att, const float* __restrict__ x,
                                                      const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                      const float* __restrict__ Wpack, const float* __restrict__ bo,
                                                      float* __restrict__ r_out, float* __restrict__ h2_out,
                                                      float* __restrict__ y_out, int R, Drop d3, Drop d4, Drop d5) {
    __shared__ __attribute__((aligned(16))) float Rs[TILE_M * LDP];
    __shared__ __attribute__((aligned(16))) float Hs[TILE_M * LDP];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * TILE_M;
    BFrag<1, 16> bf;
    {
        float4 av[4], xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256;
            const int r = r0 + (e >> 5), c = (e & 31) * 4;
            av[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            xv[q] = av[q];
            if (r < R) {
                av[q] = *reinterpret_cast<const float4*>(att + (size_t)r * D + c);
                xv[q] = *reinterpret_cast<const float4*>(x + (size_t)r * D + c);
            }
        }
        bfrag_load(bf, Wpack, D, 32 * w, 0, 0, D / 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256;
            const int rr = e >> 5, c = (e & 31) * 4;
            const int r = r0 + rr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < R) {
                const uint32_t base = (uint32_t)(r * D + c);
                v.x = av[q].x * drop_mul(d3, base) + xv[q].x;
                v.y = av[q].y * drop_mul(d3, base + 1) + xv[q].y;
                v.z = av[q].z * drop_mul(d3, base + 2) + xv[q].z;
                v.w = av[q].w * drop_mul(d3, base + 3) + xv[q].w;
                if (r_out) *reinterpret_cast<float4*>(r_out + (size_t)r * D + c) = v;      // (r, h2: null in inference mode)
            }
            *reinterpret_cast<float4*>(&Rs[rr * LDP + c]) = v;
            *reinterpret_cast<float4*>(&Hs[rr * LDP + c]) = v;
        }
    }
    __syncthreads();
    ln_tile(Hs, TILE_M, LDP, ln_g, ln_b, d4, r0);
    __syncthreads();
    if (h2_out)
        for (int e = tid; e < TILE_M * 32; e += 256) {
            const int rr = e >> 5, c = (e & 31) * 4;
            if (r0 + rr < R) *reinterpret_cast<float4*>(h2_out + (size_t)(r0 + rr) * D + c) = *reinterpret_cast<const float4*>(&Hs[rr * LDP + c]);
        }
    f32x16 acc[1];
    zero_acc(acc);
    gemm32p<1, 16>(Hs, LDP, D, Wpack, D, 32 * w, 0, acc, bf);
    const int col = 32 * w + (lane & 31);
    const float bvv = bo[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lane);
        const int gr = r0 + row;
        if (gr < R)
            y_out[(size_t)gr * D + col] = (acc[0][r] + bvv) * drop_mul(d5, (uint32_t)(gr * D + col)) + Rs[row * LDP + col];
    }
}
void launch_attn_out_fwd(const AttnOutFwdArgs& a, int R, hipStream_t s) {
    VSL_LAUNCH(k_attn_out_fwd, dim3((R + TILE_M - 1) / TILE_M), dim3(256), 0, s, a.att, a.x, a.ln_g, a.ln_b, a.Wpack, a.bo, a.r_out, a.h2_out, a.y_out, R,
               a.d3, a.d4, a.d5);
}

// =========================================================================================================
// a8 (second half) backward (:183-190):  do = dy * m5 ; dh2 = do Wo ; dr = dy + LN2^T(dh2 * m4)      (tile_bodies.hpp attn_out_bwd_tile)
// =========================================================================================================
__global__ __launch_bounds__(256) void k_attn_out_bwd(AttnOutBwdArgs a, int R) {
    __shared__ __attribute__((aligned(16))) float Gs[TILE_M * LDP];
    __shared__ __attribute__((aligned(16))) float Xs[TILE_M * LDP];
    attn_out_bwd_tile(a, nullptr, Gs, Xs, blockIdx.x * TILE_M, R);
}
void launch_attn_out_bwd(const AttnOutBwdArgs& a, int R, hipStream_t s) {
    VSL_LAUNCH(k_attn_out_bwd, dim3((R + TILE_M - 1) / TILE_M), dim3(256), 0, s, a, R);
}

// =========================================================================================================
// a14 heads (:328-337, 347-352): logits = mask_logits( Conv1D(d->1)( relu( Conv1D(2d->d)([LN(feat), x]) ) ) )
//   blockIdx.y selects start / end.  `hid` (relu output) is saved for the backward.
// =========================================================================================================
constexpr int HDP = 2 * D + 4;
__global__ __launch_bounds__(256) void k_head_fwd(HeadArgs a0, HeadArgs a1, const float* __restrict__ x,
                                                  const float* __restrict__ vmask, int R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                     // [32][HDP] = [LN(feat) | x]
    float* Hd = As + TILE_M * HDP;        // [32][LDP] relu(z)
    const HeadArgs a = blockIdx.y == 0 ? a0 : a1;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * TILE_M;
    BFrag<1, 16> bf;
    {
        float4 fv[4], xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256;
            const int r = r0 + (e >> 5), c = (e & 31) * 4;
            fv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            xv[q] = fv[q];
            if (r < R) {
                fv[q] = *reinterpret_cast<const float4*>(a.feat + (size_t)r * D + c);
                xv[q] = *reinterpret_cast<const float4*>(x + (size_t)r * D + c);
            }
        }
        bfrag_load(bf, a.W0pack, D, 32 * w, 0, 0, 2 * D / 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * 256;
            const int rr = e >> 5, c = (e & 31) * 4;
            *reinterpret_cast<float4*>(&As[rr * HDP + c]) = fv[q];
            *reinterpret_cast<float4*>(&As[rr * HDP + D + c]) = xv[q];
        }
    }
    __syncthreads();
    if (a.ln_g) {                          // transformer head: LayerNorm on the encoder features (:347-348); rnn: none
        ln_tile(As, TILE_M, HDP, a.ln_g, a.ln_b, Drop{0u, 0u, 1.f}, 0);
        __syncthreads();
    }
    if (a.lnfeat)
        for (int e = tid; e < TILE_M * 32; e += 256) {
            const int rr = e >> 5, c = (e & 31) * 4;
            if (r0 + rr < R) *reinterpret_cast<float4*>(a.lnfeat + (size_t)(r0 + rr) * D + c) = *reinterpret_cast<const float4*>(&As[rr * HDP + c]);
        }
    f32x16 acc[1];
    zero_acc(acc);
    gemm32p<1, 16>(As, HDP, 2 * D, a.W0pack, D, 32 * w, 0, acc, bf);
    const int col = 32 * w + (lane & 31);
    const float bv = a.b0[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lane);
        const int gr = r0 + row;
        const float hv = fmaxf(acc[0][r] + bv, 0.f);
        Hd[row * LDP + col] = hv;
        if (a.hid && gr < R) a.hid[(size_t)gr * D + col] = hv;      // (null in inference mode: the backward alone reads it)
    }
    __syncthreads();
    {
        const int rr = tid >> 3, sub = tid & 7;
        const float* row = Hd + rr * LDP + sub * 4;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 fv = *reinterpret_cast<const float4*>(row + 32 * j);
            const float4 wv = *reinterpret_cast<const float4*>(a.w1 + sub * 4 + 32 * j);
            d += fv.x * wv.x + fv.y * wv.y + fv.z * wv.z + fv.w * wv.w;
        }
        d = grp8_sum(d);
        const int gr = r0 + rr;
        if (sub == 0 && gr < R) a.logits[gr] = d + a.b1[0] + (1.f - vmask[gr]) * MASK_VALUE;
    }
}
void launch_head_fwd(const HeadArgs& a0, const HeadArgs& a1, const float* x, const float* vmask, int R, hipStream_t s) {
    const size_t shm = (size_t)(TILE_M * HDP + TILE_M * LDP) * sizeof(float);
    VSL_LAUNCH(k_head_fwd, dim3((R + TILE_M - 1) / TILE_M, 2), dim3(256), shm, s, a0, a1, x, vmask, R);
}

// =========================================================================================================
// heads backward (a14, :349-352): dlogit -> dz = dlogit * w1 * (hid > 0) -> [dLN(feat) | dx] = dz W0 ;
//   LN backward -> dfeat.  blockIdx.y selects start / end.
// =========================================================================================================
// `fuse` (transformer head): the END head's workgroups go on, on the tile of dfeat they have just produced, with the attention-output
// backward of the predictor encoder's second pass (k_attn_out_bwd's body) -- that gradient has no other consumer, so it never leaves the chip,
// and one kernel boundary of the dependent chain is gone (tile-local: no other workgroup's data is needed).
__global__ __launch_bounds__(256) void k_head_bwd(HeadBwdArgs a0, HeadBwdArgs a1, int R, int fuse, AttnOutBwdArgs ao) {
    __shared__ __attribute__((aligned(16))) float Gs[TILE_M * LDP];
    __shared__ __attribute__((aligned(16))) float Hs[TILE_M * LDP];
    __shared__ __attribute__((aligned(16))) float Fs[TILE_M * LDP];
    __shared__ float dl[TILE_M];
    __shared__ float red[8];
    const HeadBwdArgs a = blockIdx.y == 0 ? a0 : a1;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * TILE_M;
    BFrag<2, 8> bf;
    if (a.logits) {                        // (block-uniform) vsl_io.fused_loss: the tile's seeds from its samples' logits.  T >= 32: a tile touches at most two samples
        const int b0 = r0 / a.T, b1 = min(r0 + TILE_M - 1, R - 1) / a.T;
        const float lse0 = loss_sample_lse(a.logits + (size_t)b0 * a.T, a.T, red);
        float lse1 = lse0;
        if (b1 != b0) { __syncthreads(); lse1 = loss_sample_lse(a.logits + (size_t)b1 * a.T, a.T, red); }      // (block-uniform)
        if (tid < TILE_M) {
            const int r = r0 + tid, b = r / a.T;
            dl[tid] = r < R ? loss_ce_seed(a.logits[r], b == b0 ? lse0 : lse1, r - b * a.T, (int)a.label[b], a.cs) : 0.f;
        }
    } else
    if (tid < TILE_M) dl[tid] = r0 + tid < R ? a.dlogit[r0 + tid] : 0.f;
    load_tile128(Hs, a.hid, r0, TILE_M, R);
    load_tile128(Fs, a.feat, r0, TILE_M, R);
    bfrag_load(bf, a.W0Tpack, 2 * D, 32 * w, D, 0, D / 8);
    __syncthreads();
    for (int e = tid; e < TILE_M * 32; e += 256) {
        const int rr = e >> 5, c = (e & 31) * 4;
        const float4 hv = *reinterpret_cast<const float4*>(&Hs[rr * LDP + c]);
        const float4 wv = *reinterpret_cast<const float4*>(a.w1 + c);
        const float d = dl[rr];
        const float4 dz = make_float4(hv.x > 0.f ? d * wv.x : 0.f, hv.y > 0.f ? d * wv.y : 0.f, hv.z > 0.f ? d * wv.z : 0.f,
                                      hv.w > 0.f ? d * wv.w : 0.f);
        *reinterpret_cast<float4*>(&Gs[rr * LDP + c]) = dz;
        if (r0 + rr < R) *reinterpret_cast<float4*>(a.gz + (size_t)(r0 + rr) * D + c) = dz;
    }
    __syncthreads();
    {   // bias / w1 partials: threads 0..127 -> db0[c], 128..255 -> dw1[c]
        const int c = tid & 127;
        float acc = 0.f;
        if (tid < 128) { for (int rr = 0; rr < TILE_M; ++rr) acc += Gs[rr * LDP + c]; a.p_b0[(size_t)blockIdx.x * D + c] = acc; }
        else { for (int rr = 0; rr < TILE_M; ++rr) acc += dl[rr] * Hs[rr * LDP + c]; a.p_w1[(size_t)blockIdx.x * D + c] = acc; }
        if (tid == 0) { float sdl = 0.f; for (int rr = 0; rr < TILE_M; ++rr) sdl += dl[rr]; a.p_b1[blockIdx.x] = sdl; }
    }
    f32x16 acc[2];
    zero_acc(acc);
    gemm32p<2, 8>(Gs, LDP, D, a.W0Tpack, 2 * D, 32 * w, D, acc, bf);
    __syncthreads();                       // everyone is done reading Hs/Gs
    const int col = 32 * w + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lane);
        Hs[row * LDP + col] = acc[0][r];                           // grad wrt LN(feat)
        if (r0 + row < R) a.dx[(size_t)(r0 + row) * D + col] = acc[1][r];
    }
    __syncthreads();
    if (a.ln_g) {
        LnResid nores;
#pragma unroll
        for (int j = 0; j < 4; ++j) nores.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool go_on = fuse && blockIdx.y == 1;
        ln_bwd_tile(Hs, Fs, nores, a.ln_g, go_on ? nullptr : a.dfeat, a.p_lng, a.p_lnb, r0, R, go_on ? Gs : nullptr);
        if (go_on) {                       // (block-uniform)
            __syncthreads();               // the column sums of ln_bwd_tile are done with Hs / Fs; Gs holds dfeat (rows >= R zero)
            attn_out_bwd_tile(ao, Gs, Hs, Fs, r0, R);
        }
    } else {
        for (int e = tid; e < TILE_M * D; e += 256) {
            const int rr = e >> 7, c = e & 127;
            if (r0 + rr < R) a.dfeat[(size_t)(r0 + rr) * D + c] = Hs[rr * LDP + c];
        }
    }
}
void launch_head_bwd(const HeadBwdArgs& a0, const HeadBwdArgs& a1, int R, hipStream_t s, const AttnOutBwdArgs* fuse) {
    AttnOutBwdArgs ao;
    memset(&ao, 0, sizeof ao);
    if (fuse) ao = *fuse;
    VSL_LAUNCH(k_head_bwd, dim3((R + TILE_M - 1) / TILE_M, 2), dim3(256), 0, s, a0, a1, R, fuse ? 1 : 0, ao);
}

}  // namespace vsl
