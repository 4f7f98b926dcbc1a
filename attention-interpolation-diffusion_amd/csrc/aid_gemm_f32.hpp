// What the float32 GEMM kernels share (aid_gemm_f32_kernel in aid_f32.hip: exact fp32 MFMAs; aid_gemm_f32x3_kernel in aid_f32x3.hip:
// three bf16 products of split operands): the tile a workgroup owns, the accumulators' layout, the epilogue and the host's tile rule.
// A kernel adds what makes it different: its LDS staging, its fragment reads and its MFMA block.
//
// Tiles of FBM x FBM (128 or 64), four waves of (FBM / 2) x (FBM / 2) = NB x NB blocks of 32 x 32.  The swapped product D[n][m]
// leaves four consecutive n of one row m in a lane: acc[n block][m block][4 g + e] of lane (l31, hi) is row m0 + wm + 32 (m block) + l31,
// column n0 + wn + 32 (n block) + 8 g + 4 hi + e.
#pragma once
#include "aid_common.hpp"
#include "aid_kernels.hpp"

#include <type_traits>

namespace aid {

__device__ __forceinline__ int f32_problem_of_block(const GemmGroup& g) {
    int p = 0;
#pragma unroll
    for (int i = 1; i < AID_GEMM_MAX_PROBLEMS; ++i)
        if (i < g.n_problems && (int)blockIdx.x >= g.tile_start[i]) p = i;
    return p;
}

template <int FBM>
struct F32Tile {
    static constexpr int WT = FBM / 2, NB = WT / 32, RS = FBM / 64;           // wave tile, 32-blocks per side, staging rows per thread
    typedef f32x16 Acc[NB][NB];                                               // [n block][m block]

    const int p;                                           // block -> (problem, batch, tile)
    const GemmDesc& P;
    int batch, m0, n0;
    int l31, hi, wm, wn;                                   // lane and wave coordinates
    int srow;                                              // staging: thread -> (row = tid / 4 [+ 64], k chunk = tid % 4)

    __device__ __forceinline__ explicit F32Tile(const GemmGroup& g) : p(f32_problem_of_block(g)), P(g.p[p]) {
        int rem = blockIdx.x - g.tile_start[p];
        const int tiles_n = (P.n + FBM - 1) / FBM, tiles_m = (P.m + FBM - 1) / FBM;
        batch = rem / (tiles_m * tiles_n);
        rem -= batch * tiles_m * tiles_n;
        // column tiles of one row panel are neighbours in the grid: they share the A panel in L2
        m0 = (rem / tiles_n) * FBM;
        n0 = (rem % tiles_n) * FBM;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        l31 = lane & 31;
        hi = lane >> 5;
        wm = (wave >> 1) * WT;
        wn = (wave & 1) * WT;
        srow = tid >> 2;
    }

    // the staging rows of this thread in an A-side ([m, k]) and a B-side ([n, k]) operand, from column sq on; rows past the matrix are
    // clamped (their products are never stored)
    __device__ __forceinline__ void rows(const void* a, int64_t stride_a, int lda, const void* b, int64_t stride_b, int ldb, int sq,
                                         const float* (&ap)[RS], const float* (&bp)[RS]) const {
        const float* __restrict__ A = reinterpret_cast<const float*>(a) + (int64_t)batch * stride_a;
        const float* __restrict__ B = reinterpret_cast<const float*>(b) + (int64_t)batch * stride_b;
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            ap[i] = A + (int64_t)min(m0 + srow + 64 * i, P.m - 1) * lda + sq;
            bp[i] = B + (int64_t)min(n0 + srow + 64 * i, P.n - 1) * ldb + sq;
        }
    }

    static __device__ __forceinline__ void zero(Acc& acc) {
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    // Epilogue: every option of AidGemmProblem; fp32 needs no intermediate rounding.  LN: the group may carry a folded LayerNorm;
    // LRT = GemmLR: the problems may carry a DoRA gain (lr.p[p].row_scale).  With both off neither is compiled in.
    template <bool LN, typename LRT>
    __device__ __forceinline__ void epilogue(const Acc& acc, const LRT& lr) const {
        const GemmDesc P = this->P;                        // a copy: its fields are read once here, not again behind every store
        float* __restrict__ C = reinterpret_cast<float*>(P.c) + (int64_t)batch * P.stride_c;
        const float* stats = LN && P.ln_stats ? P.ln_stats + 2 * (int64_t)batch * P.stride_stats : nullptr;
        const float* bias = reinterpret_cast<const float*>(P.bias);
        // (laid out like C, batch stride included — aid_hip.h)
        const float* R = P.residual ? reinterpret_cast<const float*>(P.residual) + (int64_t)batch * P.stride_c : nullptr;
        const bool vec = !P.trans_rows && !stats && P.n % 4 == 0 &&     // whole 16-byte groups of a row: one store each
                         (reinterpret_cast<uintptr_t>(bias) & 15) == 0 && (reinterpret_cast<uintptr_t>(R) & 15) == 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int m = m0 + wm + 32 * j + l31;
            if (m >= P.m) continue;
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int nb = n0 + wn + 32 * i + 8 * gq + 4 * hi;
                    if (vec) {
                        if (nb >= P.n) continue;
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * gq + e] * P.scale;
                        // DoRA: gain on the weight rows, before every epilogue step.  (Here, as the accumulators leave their registers:
                        // all of them scaled at once after the K loops cost the big tile a wave of occupancy.)
                        if constexpr (std::is_same<LRT, GemmLR>::value) {
                            const GemmLRDesc& L = lr.p[p];
                            if (L.row_scale) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * gq + e];
                                lr_row_scale4(v, L.row_scale, L.side, m, nb, P.n);
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] *= P.scale;
                            }
                        }
                        if (bias) v += *reinterpret_cast<const f32x4*>(bias + nb);
                        const int64_t off = (int64_t)m * P.ldc + nb;
                        if (R) v += *reinterpret_cast<const f32x4*>(R + off);
                        *reinterpret_cast<f32x4*>(C + off) = v;
                        continue;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int n = nb + e;
                        if (n >= P.n) {                                // columns [n, round_up(n, 4)) are written with zeros (aid_hip.h)
                            if (!P.trans_rows && n < (P.n + 3) / 4 * 4) C[(int64_t)m * P.ldc + n] = 0.f;
                            continue;
                        }
                        float v = acc[i][j][4 * gq + e];
                        if constexpr (std::is_same<LRT, GemmLR>::value) {
                            const GemmLRDesc& L = lr.p[p];
                            if (L.row_scale) v *= L.row_scale[L.side == 1 ? m : n];
                        }
                        if (stats) {                                   // folded LayerNorm: rstd (x W'^T - mean colsum) + shift
                            if (P.ln_side == 1) v = fmaf(stats[2 * m + 1], fmaf(-stats[2 * m], P.ln_colsum[n], v), P.ln_shift[n]);
                            else                v = fmaf(stats[2 * n + 1], fmaf(-stats[2 * n], P.ln_colsum[m], v), P.ln_shift[m]);
                        }
                        v *= P.scale;
                        if (bias) v += bias[n];
                        int64_t off;
                        if (P.trans_rows) off = (int64_t)(m / P.trans_rows) * P.stride_c + (int64_t)n * P.ldc + m % P.trans_rows;
                        else              off = (int64_t)m * P.ldc + n;
                        if (R) v += R[off];
                        C[off] = v;
                    }
                }
        }
    }
};

// The host's tile rule (aid_f32.hip): 128 x 128 tiles (*big) only when there are enough of them to give every CU two (512 on MI355X),
// else 64 x 64; fills g.tile_start for the choice and sets *tiles (0: nothing to launch).  The K order inside a tile does not depend on
// the tile size: results are bit-identical either way.  hipErrorInvalidDevice when the device's CU count cannot be read.
hipError_t gemm_f32_tiles(GemmGroup& g, int* tiles, bool* big);

}  // namespace aid
