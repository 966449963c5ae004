// VisualProjection's data gradient (vsl_input_grads): the gradient of the loss with respect to the video features.  A unit of its own: nothing of
// vsl_forward / vsl_backward launches it, and no plan or pack knows about it.
#include "common.hpp"
#include "launch.hpp"
#include <algorithm>

namespace vsl {

// =========================================================================================================
// dX[r][c] = m(r, c) * sum_{j < 128} G[r][j] W[j][c]      G = d_video_affine (R, 128), W = the Conv1D weight (128, Dv) as the parameter
// bucket holds it, m = the multiplier the forward applied to feature (r, c): drop_keep_scale(dp, r Dv + c) mod 2^32, or 1 without dropout.
// On the fp32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain): the B operand of one k-step is ONE float of a row of W per lane --
// lane (j, h) reads W[k][c0 + j], 128 contiguous bytes per half-wave straight from the unpacked weight -- so the product needs no pack and no split
// of a weight that every workgroup would have to redo.
// A workgroup keeps its 32 rows of G (all of K = 128) in LDS and walks column blocks of 128: blockIdx.y, + gridDim.y, ...; wave w owns columns
// [32 w, 32 w + 32) of a block.  The 64 weight values a lane needs for the NEXT block are requested k-block by k-block between the MFMAs of the
// current one (two register sets used alternately), so a block's loads are a block old when they are waited for.  One barrier, after the tile load:
// a wave whose 32 columns lie beyond Dv skips the block on its own.
// A lane map (32x32x2): lane (i, h) holds G[i][k]; the float4 at k = 8 kb + 4 h feeds MFMAs q = 0..3 of k-block kb, which therefore contract
// k = 8 kb + q (lanes 0-31) and 8 kb + 4 + q (lanes 32-63): B lane (j, h) of that MFMA is W[8 kb + 4 h + q][c0 + j].  C/D: acc_row.
// =========================================================================================================
constexpr int VDX_CB = 128;             // columns per column block
struct WFrag { float b[D / 2]; };       // a lane's share of a 128 x 32 weight tile: 16 k-blocks x 4

// the four k-steps of k-block kb: a uniform row address plus the lane's own 32-bit BYTE offset `lo` = 4 ((4 h) Dv + column) -- the scalar-base
// form of global_load, no 64-bit address arithmetic per load
__device__ __forceinline__ void vdx_load_kb(WFrag& f, const float* __restrict__ W, int Dv, uint32_t lo, int kb) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        f.b[kb * 4 + q] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(W + (size_t)(kb * 8 + q) * Dv) + lo);
}

__global__ __launch_bounds__(256) void k_vproj_dx(const VprojDxArgs a) {
    __shared__ __attribute__((aligned(16))) float Gs[TILE_M * LDP];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * TILE_M, R = a.R, Dv = a.Dv, ncb = (Dv + VDX_CB - 1) / VDX_CB, ny = gridDim.y;
    // a lane's column of block cb, clamped for the loads (a column beyond Dv is computed from column Dv - 1's weights and never stored)
    auto woff = [&](int cb) { return 4u * (uint32_t)(4 * h * Dv + min(cb * VDX_CB + 32 * w + j, Dv - 1)); };
    WFrag f0, f1;
    {
        const uint32_t lo = woff(blockIdx.y);
#pragma unroll
        for (int kb = 0; kb < D / 8; ++kb) vdx_load_kb(f0, a.W, Dv, lo, kb);
    }
    load_tile128(Gs, a.G, r0, TILE_M, R);          // rows >= R: zeros
    __syncthreads();
    const float* arow = Gs + j * LDP + 4 * h;
    auto block = [&](const WFrag& cur, WFrag& nxt, int cb) {
        // (the last block of a workgroup requests its own weights once more, from the L1: straight-line code between the MFMAs, and the
        // compiler's wait counts stay exact -- behind a branch it waits for the loads it has just issued)
        const uint32_t ln = woff(cb + ny < ncb ? cb + ny : cb);
        const int c0 = cb * VDX_CB + 32 * w;
        if (c0 >= Dv) {                             // (wave-uniform) nothing of this block is this wave's: only keep the next block's weights coming
#pragma unroll
            for (int kb = 0; kb < D / 8; ++kb) vdx_load_kb(nxt, a.W, Dv, ln, kb);
            return;
        }
        f32x16 acc;                                 // ONE chain: the instruction's issue interval equals its dependent latency (64 cycles)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float4 av = *reinterpret_cast<const float4*>(arow);
        static_for<0, D / 8>([&](auto kc) {
            constexpr int kb = decltype(kc)::value;
            const float4 an = *reinterpret_cast<const float4*>(arow + (kb + 1 < D / 8 ? kb + 1 : kb) * 8);
            vdx_load_kb(nxt, a.W, Dv, ln, kb);
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, cur.b[kb * 4 + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, cur.b[kb * 4 + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, cur.b[kb * 4 + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, cur.b[kb * 4 + 3], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            av = an;
        });
        const int c = c0 + j;
        if (c < Dv) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gr = r0 + acc_row(r, lane);
                if (gr < R) {
                    float v = acc[r];
                    // the forward's element index: (size_t) r Dv + c cut to 32 bits = this product in 32-bit arithmetic
                    if (a.dp.thresh) { const float m = drop_keep_scale(a.dp, (uint32_t)gr * (uint32_t)Dv + (uint32_t)c); v = m != 0.f ? v * m : 0.f; }
                    a.dX[(size_t)gr * Dv + c] = v;
                }
            }
        }
    };
    for (int cb = blockIdx.y; cb < ncb; cb += 2 * ny) {
        block(f0, f1, cb);
        if (cb + ny < ncb) block(f1, f0, cb + ny);
    }
}

// grid: one workgroup per 32-row tile, times `ny` column phases.  ny = what brings the grid to two workgroups per CU (the second wave of a SIMD runs
// its MFMAs under the first one's stores and hashes), but never so many that a workgroup walks fewer than two column blocks: the tile of G and the
// first block's weights are loaded once per workgroup, unhidden
void launch_vproj_dx(const VprojDxArgs& a, hipStream_t s) {
    const int ntiles = (a.R + TILE_M - 1) / TILE_M, ncb = (a.Dv + VDX_CB - 1) / VDX_CB;
    const int want = a.cus > 0 ? (2 * a.cus + ntiles - 1) / ntiles : 1;
    const int ny = std::max(1, std::min(want, ncb / 2));
    VSL_LAUNCH(k_vproj_dx, dim3(ntiles, ny), dim3(NTHREADS), 0, s, a);
}

}  // namespace vsl
