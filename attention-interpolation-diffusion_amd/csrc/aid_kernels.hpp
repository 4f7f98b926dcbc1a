// Internal (C++) interfaces between the C-ABI translation unit and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/aid_hip.h"

namespace aid {

struct GemmDesc {
    const void* a;
    const void* b;
    void*       c;
    const void* bias;
    const void* residual;                             // added after the rounding of scale * A B^T + bias (NULL = none)
    int32_t m, n, k;
    int32_t lda, ldb, ldc;
    int32_t batch;
    float   scale;                                    // C = scale * A B^T + bias
    int64_t stride_a, stride_b, stride_c;
    // LayerNorm folded into the projection (AidGemmProblem.ln_*): the weight operand holds W' = W * gamma, the epilogue
    // turns  x W'^T  into  LayerNorm(x) W^T = rstd (x W'^T - mean * colsum) + shift
    const float* ln_stats;                            // [activation rows, 2] = (mean, rstd); NULL = no LayerNorm
    const float* ln_colsum;                           // [weight rows]  sum_k W'[row, k]
    const float* ln_shift;                            // [weight rows]  sum_k beta[k] W[row, k]
    int32_t ln_side;                                  // 1: the activation is A (statistics by m), 2: it is B (by n)
    int32_t trans_rows;                               // > 0: C is written transposed per frame of `trans_rows` rows (AidGemmProblem)
    int64_t stride_stats;                             // activation rows per batch
};

struct GemmGroup {                        // passed by value as the kernel argument
    GemmDesc p[AID_GEMM_MAX_PROBLEMS];
    int32_t  tile_start[AID_GEMM_MAX_PROBLEMS + 1];   // prefix sums of block counts (filled by the launcher)
    int32_t  n_problems;
    int32_t  interleave;                              // 1: every XCD gets a chunk of each problem (unequal K loops)
};

// Low-rank second K segment of a problem (AidGemmProblem.lr_*): acc += LA[m0.., 0:k] LB[n0.., 0:k]^T after the main K loop, before
// the epilogue.  Entry i belongs to GemmGroup.p[i] (k = 0: none).  The edge, lock-step, 256-row ping-pong and fp32 GEMM kernels take it as a trailing
// by-value kernel argument whose TYPE compiles the segment in: GemmLR = with the segment (the profile labels call that instantiation
// `<kernel>_lr`), NoLR = without.
struct GemmLRDesc {
    const void* a;                                    // [m, k] (row stride lda), batch b at a + b * stride_a
    const void* b;                                    // [n, k] (row stride ldb)
    int32_t k, lda, ldb;
    int32_t side;                                     // row_scale is indexed by m (1) or by n (2)
    int64_t stride_a, stride_b;
    const float* row_scale;                           // DoRA gain on the weight rows (AidGemmProblem.lr_row_scale); NULL = none
};
struct GemmLR {
    GemmLRDesc p[AID_GEMM_MAX_PROBLEMS];
};
struct NoLR {};                                       // no low-rank segment

// DoRA gain of a GemmLR problem: the accumulators of a wave (blocks [n block][m block] in the mfma32 result layout: register r of lane
// (l31, hi) is row m + 32 * (m block), column n + 32 * (n block) + 8 * (r >> 2) + (r & 3), with m / n the lane's first row / column)
// times gain[column] (side 2) or gain[row] (side 1).  Indices are clamped to the matrix; what lies past it is never stored.
// Scalar multiplies on purpose (the empty asm keeps hipcc from pairing them, see Engine::store_tile in aid_gemm.hip).
// the same for the four consecutive columns n .. n + 3 of row m (m inside the matrix) that an epilogue step holds
template <typename V4>
__device__ __forceinline__ void lr_row_scale4(V4& v, const float* __restrict__ gain, int side, int m, int n, int N) {
    const float gm = gain[side == 1 ? m : min(n, N - 1)];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = v[e] * (side == 1 || e == 0 ? gm : gain[min(n + e, N - 1)]);
        asm volatile("" : "+v"(t));
        v[e] = t;
    }
}
template <int NB, int MB, typename ACC>
__device__ __forceinline__ void lr_row_scale(ACC (&acc)[NB][MB], const float* __restrict__ gain, int side, int m, int n, int M, int N) {
    if (side == 1) {
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            const float gm = gain[min(m + 32 * j, M - 1)];
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float t = acc[i][j][r] * gm;
                    asm volatile("" : "+v"(t));
                    acc[i][j][r] = t;
                }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gn = gain[min(n + 32 * i + 8 * gq + e, N - 1)];
#pragma unroll
                    for (int j = 0; j < MB; ++j) {
                        float t = acc[i][j][4 * gq + e] * gn;
                        asm volatile("" : "+v"(t));
                        acc[i][j][4 * gq + e] = t;
                    }
                }
    }
}

// CU count of the current device, read once per device; 0 when there is no device or the query fails (aid_gemm.hip)
int device_cu_count();

// fills g.tile_start (the kernels' block -> problem map) in units of bm x bn tiles and returns the tile count (aid_gemm.hip)
int fill_tile_start(GemmGroup& g, int bm, int bn);

// Side problems of a ping-pong launch: the few short problems of a group whose K loop differs from the main ones (the
// K = 2048 text-context projections next to the K = 1280 query projection of a cross-attention layer).  They run as
// 128 x 128 lock-step tiles in the FIRST blocks of the same launch, so the main problems keep the big-tile engine.
struct GemmSide {
    GemmDesc p[4];
    int32_t  tile_start[5];               // prefix sums of 128 x 128 tile counts
    int32_t  n;                           // number of side problems (0 = none)
    int32_t  tiles;                       // total side tiles
    int32_t  pad_tiles;                   // tiles rounded up to a multiple of 8 (keeps block -> XCD of the main tiles)
};

// Development / tuning knobs.  They are NOT read from the environment in the launch path: the table is filled once when
// the library is loaded (environment variables AID_<NAME>, e.g. AID_ATTN_NW=8) and can be changed at run time through
// aid_set_tuning() — same-process A/B runs flip a knob between launches.  -1 = unset (the launch heuristics decide).
enum Tune {
    TUNE_GEMM_VARIANT = 0,      // 7 = force the lock-step engine, 31 = force the ping-pong engine
    TUNE_GEMM_PP,               // ping-pong K loop: 0 = DMA issued between the MFMAs, 1 = in the read slot, 2 = 1 + s_setprio; 3 = the default (1)
    TUNE_GEMM_TRI,              // 0 = never use the twelve-wave 288 x 256 engine, 1 = force it where the shape allows
    TUNE_ATTN_NW,               // 4 / 8 waves per workgroup
    TUNE_ATTN_QB,               // 1 / 2 query blocks per wave (d = 40 PLAIN)
    TUNE_ATTN_PIPE,             // 0 / 1 software-pipelined loop; ping-pong kernel: 0 = one item per workgroup (no persistent walk) — and with
                                // that the default rule keeps PLAIN calls below 2048 keys off the ping-pong kernel (attn_pp_persistent)
    TUNE_ATTN_RES,              // 0 / 1 resident key segments
    TUNE_ATTN_RES_CHUNKS,       // > 0: chunks per (frame, head) of the resident variant
    TUNE_ATTN_ORDER,            // 0 = plain XCD order for mixed launches
    TUNE_ATTN_V2,               // ping-pong d = 64 kernel: 0 never / 1 wherever supported; default: fused OUTER / INNER l >= 1024, PLAIN l >= 1024 on persistent workgroups, everything else l >= 2048
    TUNE_CU_SHARE,              // n > 1: the caller runs n independent launch streams side by side (two passes on two streams): the GEMM
                                // engine choice plans with 1 / n of the CUs; a hint, results never depend on it
    TUNE_GEMM_RS,               // row-stationary engine for the short-K levels (aid_gemm_rs.hip): 0 = never, 1 = wherever the shape allows;
                                // default: wherever the shape allows AND the activation has enough row tiles to fill the device
    TUNE_ATTN_TX,               // text-key kernel (aid_attn_tx.hip: d = 64, <= 96 keys per segment, PLAIN / INNER / OUTER): 0 = never; default: wherever supported
    TUNE_ATTN_TX_TILES,         // > 0: 32-row tiles per wave of that kernel (sets the workgroups per (frame, head))
    TUNE_GEMM_LS,               // ring of the lock-step engine: 0 = 2 stages of 64 k, 2 workgroups / CU (rounds 1 - 5); 1 = 4 stages of 64 k,
                                // 1 workgroup / CU; default: 1 for launches of at most one workgroup per CU with >= 16 K tiles (aid_gemm.hip)
    TUNE_GEMM_LR_PP,            // groups with low-rank segments on the 256-row ping-pong engine: 0 = never (lock-step / edge), 1 = wherever the shape
                                // allows, 2 = the cost model with the segment's K tiles counted (plan_gemm); default: 0, until 2 is measured
    TUNE_COUNT
};
int tune(int id);

// picks the engine and launches it; `variant` / `symbol` receive the engine's name and its kernel symbol
// cu_share > 1: the caller runs that many launch streams side by side (AidGemmProblem.cu_share); 0 / 1: the process-wide CU_SHARE knob decides
// lr (optional): low-rank segments of the problems; a group with any lr->p[i].k > 0 runs on an engine that carries them (edge, lock-step, 256-row ping-pong)
hipError_t gemm_group_launch(GemmGroup& g, int dtype, hipStream_t stream, const char** variant = nullptr, const char** symbol = nullptr,
                             int cu_share = 0, GemmLR* lr = nullptr);

// row-stationary engine (aid_gemm_rs.hip): K = 320 / 640, one shared tall activation; `ncu` = CUs the launch may count on
bool       gemm_rs_supported(const GemmGroup& g, int ncu, bool ignore_size);
hipError_t gemm_rs_launch(const GemmGroup& g, int dtype, int ncu, hipStream_t stream);

// float32 storage path (aid_f32.hip)
hipError_t gemm_f32_launch(GemmGroup& g, hipStream_t stream, const GemmLR* lr = nullptr);
// the same GEMM with every operand element split into two bf16 halves, three bf16 products (aid_f32x3.hip; AidGemmProblem.f32_split);
// plain groups only: no low-rank segment, no folded LayerNorm
hipError_t gemm_f32x3_launch(GemmGroup& g, hipStream_t stream);
hipError_t attn_f32_launch(const AidAttnArgs& a, hipStream_t stream);
// the same core with both products from bf16 halves (aid_f32x3.hip; AidAttnArgs.f32_split): d = 40 / 64 / 80, every mode and option
bool       attn_f32x3_supported(const AidAttnArgs& a);
hipError_t attn_f32x3_launch(const AidAttnArgs& a, hipStream_t stream);
hipError_t lerp_kv_f32_launch(const void* k, const void* vt, void* k2, void* vt2, const float* coef, int n_frames, int begin,
                              int end, int64_t k_fs, int64_t vt_fs, hipStream_t stream);

// attention core: plan_attn picks the kernel(s) of a call and launches nothing; launch_attn_plan runs one step of the plan (aid_attn.hip)
enum class AttnEngine { F32, Tx, Pp, Order };         // aid_f32.hip / aid_f32x3.hip, aid_attn_tx.hip, aid_attn_pp.hip, aid_attn_kernel (program order)
enum class AttnShare { All = 0, Single = 1, Rest = 2 };   // what a step runs: the whole call; the frames with ONE key segment; the others
struct AttnStep {
    AttnEngine engine = AttnEngine::Order;
    AttnShare  share = AttnShare::All;                // Pp + Single, then Order + Rest (AttnKParams.skip_single): the two launches of a split call
    int  nw = 4, qb = 1;                              // Order, the variant: waves per workgroup, 32-row query blocks per wave, software-
    bool pipe = false, res = false, bias = false;     //   pipelined loop, resident key segments, score bias (at most one differs from these)
    bool split = false;                               // F32: the three-term bf16 kernel (aid_attn_f32x3_kernel)
    int  nqb = 0, q_iters = 1;                        // Order: workgroups per (frame, head), query blocks each works through
    char label[64] = "";                              // profile entry (AidProfileEntry.kernel)
};
struct AttnPlan {
    int      n_steps = 1;
    AttnStep step[2];
    int      n_single = 0;                            // frames of the call with ONE key segment (work attribution of a split call)
    char     variant[64] = "";                        // aid_last_attn_variant()
};
AttnPlan   plan_attn(const AidAttnArgs& a);
hipError_t launch_attn_plan(const AidAttnArgs& a, const AttnStep& st, hipStream_t stream);
// d = 64 ping-pong kernel for the single-segment frames of a call (aid_attn_pp.hip); frames with more segments exit at once
bool       attn_pp_supported(const AidAttnArgs& a);
hipError_t attn_pp_launch(const AidAttnArgs& a, hipStream_t stream, bool multi);
// that launch as one persistent workgroup per CU (more items than CUs, whole 8-tile trips); *n_cu: the device's CUs (256 when they cannot be read)
bool       attn_pp_persistent(const AidAttnArgs& a, bool multi, int* n_cu);
// d = 64 kernel for TEXT keys (<= 96 keys per segment resident in LDS; aid_attn_tx.hip): whole PLAIN / INNER / OUTER calls
bool       attn_tx_supported(const AidAttnArgs& a);
hipError_t attn_tx_launch(const AidAttnArgs& a, hipStream_t stream);
bool       attn_head_dim_supported(int d);
// IP-Adapter image segments accumulated into `out` in one launch (aid_attn_ip.hip; aid_ip_attn_fwd): 16-bit dtypes, arguments checked by the caller
hipError_t ip_attn_launch(const AidIpAttnArgs& a, hipStream_t stream);
hipError_t lerp_kv_launch(const void* k, const void* vt, void* k2, void* vt2, const float* coef, int n_frames, int begin,
                          int end, int64_t k_fs, int64_t vt_fs, int dtype, hipStream_t stream);
// end-point K / V^T rows between a call and slot *step of the end-point store (aid_endpoint.hip); arguments checked by the caller
hipError_t endpoint_rows_launch(const AidEndpointRows& a, hipStream_t stream);
// key-frame K / V^T rows between a call and slot *step of up to AID_KF_MAX_ROWS key-frame stores (aid_keyframe.hip); arguments checked
// by the caller
hipError_t keyframe_rows_launch(const AidKeyframeRows& a, hipStream_t stream);
// the same rows between a call and 8-bit block stores, quantised on PUT and dequantised on GET (aid_keyframe_q8.hip); arguments
// checked by the caller
hipError_t keyframe_rows_q8_launch(const AidKeyframeRowsQ8& a, hipStream_t stream);
// corner-weighted AID (aid_corners.hip): the INNER mix among up to AID_MAX_CORNERS rows of k / vt into the first n_mix rows of
// k2 / vt2, and the pair table of aid_attn_corners_fwd ([1 + 2 ceil(M / 2), n_frames] floats); arguments checked by the caller
struct CornerRows { int32_t row[AID_MAX_CORNERS]; };          // by value in the kernel arguments
hipError_t mix_kv_launch(const void* k, const void* vt, void* k2, void* vt2, const float* w, const CornerRows& rows, int n_corners,
                         int n_mix, int64_t k_fs, int64_t vt_fs, int dtype, hipStream_t stream);
hipError_t corner_pairs_launch(const float* w, float* tab, int n_frames, int n_mix, int n_corners, hipStream_t stream);
// the same mix with block row *step of n_corners key-frame stores as the corners (aid_keyframe_blend.hip; aid_mix_kv_stores);
// arguments checked by the caller
struct MixStoresArgs {
    const AidKeyframeRow* rows;                       // HOST: n_corners entries (`row` not read)
    const int32_t* step;                              // DEVICE
    const float*   weights;                           // DEVICE [n_mix (+ riders), n_corners]
    void *k2, *vt2;
    int32_t n_corners, n_steps, q8, n_mix;
    int64_t k_fs, vt_fs;
    int32_t vt_ld, vt_cols, dtype;                    // vt_ld / vt_cols: q8 only
};
hipError_t mix_kv_stores_launch(const MixStoresArgs& a, hipStream_t stream);
hipError_t layernorm_launch(const void* x, const void* gamma, const void* beta, void* y, int64_t rows, int c, float eps,
                            int dtype, hipStream_t stream);
hipError_t ln_stats_launch(const void* x, float* stats, int64_t rows, int c, float eps, int dtype, hipStream_t stream);
hipError_t ln_fold_launch(const void* w, const void* gamma, const void* beta, void* w_folded, float* colsum, float* shift,
                          int rows, int c, int dtype, hipStream_t stream);
// DoRA row gain (aid_dora.hip): gain[n] = magnitude[n] / ||W[n, :] + (B_pack A_pack)[n, :]||
hipError_t dora_gain_launch(const void* w, const void* a_pack, const void* b_pack, const void* magnitude, float* gain, int n_out,
                            int n_in, int ldw, int rank, int dtype, hipStream_t stream);
// classifier-free guidance + guidance rescale, one workgroup per sample (aid_cfg.hip); arguments checked by the caller
hipError_t cfg_rescale_launch(const void* text, const void* uncond, void* out, int n, int64_t e, int64_t text_stride,
                              int64_t uncond_stride, int64_t out_stride, float gs, float phi, int dtype, hipStream_t stream);
bool       layernorm_width_supported(int c);

}  // namespace aid
