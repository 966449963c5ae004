// Parameter-buffer kernels of the VSLNet hot path (gfx950): weight packing in front of a forward, the reduction of the backward's partial slabs into
// the flat gradient bucket (deterministic, no float atomics on global memory), and the clip + AdamW step on the flat buckets.
#include "common.hpp"
#include "launch.hpp"
#include <algorithm>

namespace vsl {

// =========================================================================================================
// weight packing (one launch per forward; jobs table lives in the plan)
// =========================================================================================================
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ params, float* __restrict__ pack,
                                              const PackJob* __restrict__ jobs) {
    const PackJob j = jobs[blockIdx.y];
    if (j.transpose == 5) {         // bf16 forward pack (round to nearest even), K zero-padded to 16
        const int kn16 = (j.kn + 15) & ~15;
        uint16_t* p16 = reinterpret_cast<uint16_t*>(pack + j.dst);
        for (int e = blockIdx.x * 256 + threadIdx.x; e < kn16 * j.cn; e += gridDim.x * 256) {
            const int c = e / kn16, k = e - c * kn16;
            const float v = k < j.kn ? params[j.src + (size_t)c * j.ld + k] : 0.f;
            p16[((size_t)(k >> 4) * j.ncols + c) * 16 + (k & 15)] = f32_to_bf16(v);
        }
        return;
    }
    if (j.transpose == 6 || j.transpose == 7) {     // split pack: three bf16 planes of the operand's terms, K zero-padded to 16
        const int kn16 = j.kfill ? j.kfill : (j.kn + 15) & ~15;     // (a job that is not the last k segment of its operand has kn % 16 == 0)
        uint16_t* p16 = reinterpret_cast<uint16_t*>(pack + j.dst);
        const size_t plane = pack3_plane(j.ktot ? j.ktot : j.kn, j.ncols);
        for (int e = blockIdx.x * 256 + threadIdx.x; e < kn16 * j.cn; e += gridDim.x * 256) {
            int c, k;
            float v = 0.f;
            if (j.transpose == 6) { c = e / kn16; k = e - c * kn16; if (k < j.kn) v = params[j.src + (size_t)c * j.ld + k]; }       // Bm[k][c] = W[c][k]
            else { k = e / j.cn; c = e - k * j.cn; if (k < j.kn) v = params[j.src + (size_t)k * j.ld + c]; }                        // Bm[k][c] = W[k][c]
            uint16_t th, tm, tl;
            split3_scalar(v, th, tm, tl);
            const size_t o = pack3_index(j.k_off + k, j.col_off + c, j.ncols);
            p16[o] = th; p16[plane + o] = tm; p16[2 * plane + o] = tl;
        }
        return;
    }
    const int kn8 = j.transpose == 0 ? (j.kn + 7) & ~7 : j.kn;     // forward pack: zero the k rows that pad the last 8-block
    const int n = kn8 * j.cn;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        int k, c;
        float v;
        if (j.transpose == 3) {     // char-conv weight (nch, char_dim, 1, kw) -> image [ci][4 taps][100 channels]
            // kn = nch * char_dim * 4 (every tap slot written: zero beyond the kernel width) ; ld = kw ; ncols = char_dim ;
            // col_off = first channel of this conv
            const int kw = j.ld, cd = j.ncols;
            const int ch = e / (cd * 4), t = e - ch * cd * 4;
            const int ci = t >> 2, kk = t & 3;
            pack[j.dst + (ci * 4 + kk) * 100 + j.col_off + ch] = kk < kw ? params[j.src + (ch * cd + ci) * kw + kk] : 0.f;
            continue;
        }
        if (j.transpose == 8) {     // char-conv weight -> B operands of k_embed_bwd's dCe product in lane order: [channel tile][76 k-steps][64 lanes]
            // kn = channel tiles * 76 * 64 ; ld = kw ; ncols = char_dim ; col_off = first channel of this conv ; k_off = its channel count.
            // k-step q covers tap eb_tap(q), channels eb_oc0(q) + (lane >> 4); this job writes the slots of ITS channels (zero where the
            // tap lies beyond the kernel width or the input channel beyond char_dim), the four jobs together define the whole image
            const int kw = j.ld, cd = j.ncols;
            const int ct = e / (EB_IMG_Q * 64), rem = e - ct * EB_IMG_Q * 64, q = rem >> 6, ln = rem & 63;
            const int kk = q < 25 ? 0 : q < 48 ? 1 : q < 66 ? 2 : 3;
            const int oc = (q < 25 ? 4 * q : q < 48 ? 8 + 4 * (q - 25) : q < 66 ? 28 + 4 * (q - 48) : 60 + 4 * (q - 66)) + (ln >> 4);
            const int ocl = oc - j.col_off, ci = 16 * ct + (ln & 15);
            if (ocl >= 0 && ocl < j.k_off) pack[j.dst + e] = (ci < cd && kk < kw) ? params[j.src + (ocl * cd + ci) * kw + kk] : 0.f;
            continue;
        }
        if (j.transpose == 9 || j.transpose == 10) {     // a (512, 128) LSTM weight in the register order of the one-sample kernels: [wave][float4 q][lane][x]
            const int x = e & 3, ln = (e >> 2) & 63, q = (e >> 8) & 31, wv = e >> 13;
            const int r = q >> 3, kk = 4 * (q & 7) + x;                       // the lane's output r (named own ^ r), its contraction index kk of 32
            const int u = 16 * wv + (ln >> 2), jj = ln & 3;
            // forward: gate (jj ^ r) of unit u at k = 32 jj + kk ; backward: gate row 32 (ln & 15) + kk, column of unit 16 wv + 4 (ln >> 4) + (quad ^ r)
            const int src = j.transpose == 9 ? ((jj ^ r) * D + u) * D + 32 * jj + kk
                                             : (32 * (ln & 15) + kk) * D + 16 * wv + 4 * (ln >> 4) + (((ln >> 2) & 3) ^ r);
            pack[j.dst + e] = params[j.src + src];
            continue;
        }
        if (j.transpose == 4) {     // zero fill of kn * cn floats
            pack[j.dst + e] = 0.f;
            continue;
        }
        if (j.transpose) {          // Bm[k][c] = W[k][c]  (W row = contraction index): c is the fast source index
            k = e / j.cn; c = e - k * j.cn;
            v = params[j.src + (size_t)k * j.ld + c];
        } else {                    // Bm[k][c] = W[c][k]: k is the fast source index
            c = e / kn8; k = e - c * kn8;
            v = k < j.kn ? params[j.src + (size_t)c * j.ld + k] : 0.f;
        }
        pack[j.dst + pack_index(j.k_off + k, j.col_off + c, j.ncols)] = v;
    }
}
void launch_pack(const float* params, float* pack, const PackJob* jobs_dev, int njobs, hipStream_t s) {
    if (njobs == 0) return;
    VSL_LAUNCH(k_pack, dim3(64, njobs), dim3(256), 0, s, params, pack, jobs_dev);
}

// =========================================================================================================
// final reduction of all partial slabs into the flat gradient bucket
// =========================================================================================================
// unit = 256 destination elements: 64 float4 lanes x 4 slab groups (group g sums slabs s = g, g + 4, ...), each
// thread keeps 8 independent 16-byte loads in flight; the 4 group sums are combined through LDS.
// sq[unit] = sum of squares of the unit's 256 results (also returned, valid in thread 0): every gradient of the bucket leaves this code, so the
// clip's global norm needs no pass of its own over the bucket (vsl_adamw.norm_from_backward; k_adamw adds the partials in unit order).
// ACC (vsl_backward_accumulate): the slab sum is formed exactly as without it -- same groups, same order, same LDS combine -- and the bucket's
// previous value is added LAST, one fp32 add per element: the stored value is prev + sum, and sq[unit] the sum of squares of the STORED values, so
// the norm k_adamw takes behind the last micro-batch is that of the whole accumulated bucket.  Only elements the plain form writes are read.
template <bool ACC>
__device__ __forceinline__ float reduce_unit(const float* __restrict__ ws, float* __restrict__ grads, const ReduceSeg* __restrict__ segs,
                                             const int* __restrict__ blk2seg, float* __restrict__ sq, int unit, float4 (&part)[4][64]) {
    const int si = blk2seg[2 * unit], off = blk2seg[2 * unit + 1];
    const ReduceSeg* __restrict__ sgp = segs + si;
    const int n = sgp->n, nsrc = sgp->nsrc, rl = sgp->rl, ds = sgp->ds, dst = sgp->dst;
    const int l4 = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int i = off + l4 * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sgp->vec) {
        if (i < n) {
            for (int q = 0; q < nsrc; ++q) {
                if (i >= sgp->vn[q]) continue;                       // this source covers only the first vn elements
                const float* p = ws + sgp->src[q] + i;
                const size_t ss = (size_t)sgp->ss[q];
                const int ns = sgp->nslabs[q];
                int s = grp;
                for (; s + 60 < ns; s += 64) {                       // 16 slabs of this group per iteration (the 256-slab units of the embedding backward)
                    float4 v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(s + 4 * u) * ss);
#pragma unroll
                    for (int u = 0; u < 16; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
                }
                for (; s + 28 < ns; s += 32) {                       // 8 slabs
                    float4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(s + 4 * u) * ss);
#pragma unroll
                    for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
                }
                for (; s < ns; s += 4) {
                    const float4 a = *reinterpret_cast<const float4*>(p + (size_t)s * ss);
                    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
                }
            }
        }
        part[grp][l4] = acc;
        __syncthreads();
        if (grp == 0 && i < n) {
            const float4 b1 = part[1][l4], b2 = part[2][l4], b3 = part[3][l4];
            acc.x += (b1.x + b2.x) + b3.x; acc.y += (b1.y + b2.y) + b3.y; acc.z += (b1.z + b2.z) + b3.z; acc.w += (b1.w + b2.w) + b3.w;
            if constexpr (ACC) {
                const float4 pv = *reinterpret_cast<const float4*>(grads + dst + (i / rl) * ds + (i % rl));
                acc.x = pv.x + acc.x; acc.y = pv.y + acc.y; acc.z = pv.z + acc.z; acc.w = pv.w + acc.w;
            }
            *reinterpret_cast<float4*>(grads + dst + (i / rl) * ds + (i % rl)) = acc;
        } else acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float q = 0.f;
        if (grp == 0) {                                  // (wave 0)
            q = wave_sum((acc.x * acc.x + acc.y * acc.y) + (acc.z * acc.z + acc.w * acc.w));
            if (l4 == 0) sq[unit] = q;
        }
        return q;
    } else {
        // ragged / unaligned segments (single biases, the 10- and 30-channel char-conv biases ...): same structure with
        // scalar loads -- 64 elements per pass, 4 slab groups, 8 loads in flight (a serial walk over up to 256 slabs is
        // 256 exposed memory latencies)
        float* sp = reinterpret_cast<float*>(&part[0][0]);
        float q2 = 0.f;
#pragma unroll
        for (int base = 0; base < 256; base += 64) {
            const int e = off + base + l4;
            float a = 0.f;
            if (e < n) {
                for (int q = 0; q < nsrc; ++q) {
                    if (e >= sgp->vn[q]) continue;
                    const float* p = ws + sgp->src[q] + e;
                    const size_t ss = (size_t)sgp->ss[q];
                    const int ns = sgp->nslabs[q];
                    int s = grp;
                    for (; s + 28 < ns; s += 32) {
                        float v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(s + 4 * u) * ss];
#pragma unroll
                        for (int u = 0; u < 8; ++u) a += v[u];
                    }
                    for (; s < ns; s += 4) a += p[(size_t)s * ss];
                }
            }
            __syncthreads();
            sp[grp * 64 + l4] = a;
            __syncthreads();
            if (grp == 0 && e < n) {
                float r = (sp[l4] + sp[64 + l4]) + (sp[128 + l4] + sp[192 + l4]);
                if constexpr (ACC) r = grads[dst + (e / rl) * ds + (e % rl)] + r;
                grads[dst + (e / rl) * ds + (e % rl)] = r;
                q2 += r * r;
            }
        }
        if (grp == 0) {
            q2 = wave_sum(q2);
            if (l4 == 0) sq[unit] = q2;
        }
        return q2;
    }
}
__global__ __launch_bounds__(256) void k_reduce(const float* __restrict__ ws, float* __restrict__ grads,
                                                const ReduceSeg* __restrict__ segs, const int* __restrict__ blk2seg,
                                                float* __restrict__ sq) {
    __shared__ float4 part[4][64];
    (void)reduce_unit<false>(ws, grads, segs, blk2seg, sq, blockIdx.x, part);
}
__global__ __launch_bounds__(256) void k_reduce_acc(const float* __restrict__ ws, float* __restrict__ grads,
                                                    const ReduceSeg* __restrict__ segs, const int* __restrict__ blk2seg,
                                                    float* __restrict__ sq) {
    __shared__ float4 part[4][64];
    (void)reduce_unit<true>(ws, grads, segs, blk2seg, sq, blockIdx.x, part);
}
void launch_reduce(const float* partial, float* grads, const ReduceSeg* segs_dev, const int* blk2seg_dev, int nblocks,
                   float* sq, bool accumulate, hipStream_t s) {
    if (accumulate) VSL_LAUNCH(k_reduce_acc, dim3(nblocks), dim3(256), 0, s, partial, grads, segs_dev, blk2seg_dev, sq);
    else VSL_LAUNCH(k_reduce, dim3(nblocks), dim3(256), 0, s, partial, grads, segs_dev, blk2seg_dev, sq);
}

// =========================================================================================================
// optimizer step on the flat buckets (main_t7.py:111-112, VSLNet_t7.py:8-17): HBM-bound, 5 streams of n floats.
//   k_sqsum : OPT_BLOCKS partial sums of grads^2 (grid-stride, float4), fixed summation order -- skipped when the caller vouches that
//             `grads` is what vsl_backward left (vsl_adamw.norm_from_backward): k_reduce's per-block partials are used instead
//   k_adamw : every block re-reduces the partials (L2-resident, fixed order) -> clip factor, then updates its elements
// =========================================================================================================
__global__ __launch_bounds__(256) void k_sqsum(const float* __restrict__ g, int64_t n4, float* __restrict__ partials) {
    __shared__ float red[4];
    float s = 0.f;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = g4[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// clip + AdamW of one element (main_t7.py:111-112; eps 1e-6, decoupled decay)
__device__ __forceinline__ void adamw_elem(float& pe, float& me, float& ve, float ge, unsigned char dke, float coef, const AdamHp& hp) {
    const float lr = hp.lr, b1 = hp.b1, b2 = hp.b2, step_size = hp.lr / hp.bc1;
    ge *= coef;
    if (!hp.hf_order) pe *= 1.0f - lr * (dke ? hp.wd : 0.f);
    me = b1 * me + (1.0f - b1) * ge;
    ve = b2 * ve + (1.0f - b2) * ge * ge;
    if (!hp.hf_order) pe -= step_size * me / (sqrtf(ve) / hp.bc2_sqrt + hp.eps);
    else {                                   // transformers.AdamW: eps outside the bias correction, decay after the update
        pe -= step_size * hp.bc2_sqrt * me / (sqrtf(ve) + hp.eps);
        pe -= lr * (dke ? hp.wd : 0.f) * pe;
    }
}
__device__ __forceinline__ void adamw_vec4(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const uint8_t* __restrict__ decay,
                                           int64_t i4, const float4 gv, float coef, const AdamHp& hp) {
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4 pv = p4[i4], mv = m4[i4], vv = v4[i4];
    const uchar4 dk = reinterpret_cast<const uchar4*>(decay)[i4];
    adamw_elem(pv.x, mv.x, vv.x, gv.x, dk.x, coef, hp); adamw_elem(pv.y, mv.y, vv.y, gv.y, dk.y, coef, hp);
    adamw_elem(pv.z, mv.z, vv.z, gv.z, dk.z, coef, hp); adamw_elem(pv.w, mv.w, vv.w, gv.w, dk.w, coef, hp);
    p4[i4] = pv; m4[i4] = mv; v4[i4] = vv;
}
// float4 elements [first, n4) with stride `stride`
__device__ __forceinline__ void adamw_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           const uint8_t* __restrict__ decay, int64_t first, int64_t stride, int64_t n4, float coef, const AdamHp& hp) {
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = first; i < n4; i += stride) adamw_vec4(p, m, v, decay, i, g4[i], coef, hp);
}
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, const uint8_t* __restrict__ decay, const float* __restrict__ partials,
                                               int np, int64_t n4, float clip, AdamHp hp, float* __restrict__ norm_out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < np; k += 256) s += partials[k];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
    const float coef = clip > 0.f ? fminf(1.0f, clip / (norm + 1e-6f)) : 1.0f;       // clip_grad_norm_
    adamw_span(p, g, m, v, decay, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256, n4, coef, hp);
}

void launch_adamw(const AdamwArgs& a, hipStream_t s) {
    const int64_t n4 = a.n / 4;                  // the bucket is a multiple of 4 floats (every tensor is 16-byte aligned)
    if (!a.sq_from_backward) VSL_LAUNCH(k_sqsum, dim3(OPT_BLOCKS), dim3(256), 0, s, a.grads, n4, a.partials);
    const int nb = (int)std::min<int64_t>(1024, (n4 + 255) / 256);
    VSL_LAUNCH(k_adamw, dim3(nb), dim3(256), 0, s, a.params, a.grads, a.m, a.v, a.decay_mask, a.sq_from_backward ? a.sq_from_backward : (const float*)a.partials,
               a.sq_from_backward ? a.nsq : OPT_BLOCKS, n4, a.clip, a.hp, a.norm_out);
}

}  // namespace vsl
