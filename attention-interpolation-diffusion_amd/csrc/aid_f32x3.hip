// float32 GEMM at `torch.set_float32_matmul_precision("high")` (AidGemmProblem.f32_split = 1): float32 tensors in and out,
// every operand element taken as the sum of TWO bfloat16 numbers and the product formed from three bf16 matrix products,
//     x = xh + xl,   xh = bf16_rne(x),   xl = bf16_rne(x - float(xh))          (the subtraction is exact in fp32)
//     A B^T ~= Ah Bh^T + Al Bh^T + Ah Bl^T                                       (Al Bl^T, ~2^-16 of the result, is dropped)
// on `v_mfma_f32_32x32x16_bf16` (products exact, fp32 accumulation): a third of the bf16 matrix rate instead of the fp32 vector rate
// `v_mfma_f32_32x32x2_f32` runs at (1 / 16 of the bf16 rate).  The two halves carry 16 significand bits of the 24, so a product
// is good to ~2^-16 relative per element and a GEMM with random signs to ~4e-6 rel-L2, independent of K — between
// exact fp32 (3e-7) and fp16 operands (3e-4).  bf16 halves keep the fp32 exponent range (an fp16 split would not).  Inf / NaN: an
// infinite or over-range element (|x| > 3.39e38 rounds xh to inf) gives NaN where the exact kernel gives inf.
//
//   aid_gemm_f32x3_kernel   C = scale * A B^T (+ bias) (+ residual) on the frame it shares with aid_gemm_f32_kernel (aid_gemm_f32.hpp:
//                           GemmGroup walk, edge clamping, epilogue with batches, strides, trans_rows, zeroed pad columns and 16-byte
//                           stores, the host's tile rule) and with that kernel's staging scheme (global -> registers -> LDS, the next
//                           K tile's loads in flight during the MFMAs, two LDS buffers, one barrier per K tile).  Here: the split, the
//                           four-plane LDS staging, the fragment reads and the three-term MFMA block.  No low-rank segment and no
//                           folded LayerNorm — groups that carry either run on aid_gemm_f32_kernel (aid_abi.hip)
//                           [attn.to_q / to_k / to_v / to_out[0], interpolation.py:613, 623-624, 666]
#include "aid_gemm_f32.hpp"

namespace aid {

typedef Vec<bf16>::v8 bf16x8;

// ------------------------------------------------------------------------------------------------
// 128 x 128 x 32 / 64 x 64 x 32 tiles, four waves of 64 x 64 / 32 x 32, K tiles of 32 = two k-steps of the 16-deep instruction.
//   * the split happens on the way into LDS: a thread loads 8 consecutive k of a row (two 16-byte loads), rounds them to the high
//     plane with v_cvt_pk_bf16_f32 (RNE), subtracts the high halves taken back through their BITS (a shift, not a conversion the
//     compiler could reason about under -ffast-math) and rounds the remainders to the low plane: ~100 VALU instructions per thread and
//     K tile next to 24 MFMAs of 32 cycles per wave.  No extra launch, no workspace, no cache to invalidate.
//   * LDS: four planes (A high, A low, B high, B low) of rows of 32 + 8 bf16 = 80 bytes, the fp32 kernel's row pitch: row r starts at
//     bank 20 r mod 64 — 16 distinct multiples of 4 over the 16 rows of a `ds_read_b128` lane group and over the 2 x 4 (row, chunk)
//     lanes of a `ds_write_b128` group: the 16-byte fragment reads and the 16-byte staging writes are conflict-free.
//   * `v_mfma_f32_32x32x16_bf16`: the lower lane half supplies k = 0 .. 7 of a k-step and the upper half k = 8 .. 15, ONE 16-byte
//     read per plane and fragment; the swapped product D[n][m] leaves four consecutive n of one row m in a lane (16-byte stores).
//   * per (n block, m block) and k-step the three products run low-order terms first: Bl Ah, Bh Al, Bh Ah.
// LDS per workgroup: 2 buffers x (FBM + FBN) rows x 2 planes x 80 bytes = 80 KB (128) / 40 KB (64): two workgroups of the big tile
// fill the CU's 160 KB, i.e. two waves per SIMD, which is also what the 64 accumulator + 32 fragment + 32 staging registers allow for.
// ------------------------------------------------------------------------------------------------
constexpr int XBK = 32, XLD = XBK + 8;                     // k per tile, LDS row pitch in bf16

// x0 | x1 = 8 consecutive k -> their high and low bf16 halves
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, bf16x8& h, bf16x8& l) {
    f32x8 x;
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = x0[e]; x[4 + e] = x1[e]; }
    h = cvt8<bf16>(x);
    const u32x4 hb = __builtin_bit_cast(u32x4, h);         // element 2 i in the low 16 bits of word i, 2 i + 1 in the high 16
    f32x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[2 * i]     = x[2 * i]     - __uint_as_float(hb[i] << 16);
        r[2 * i + 1] = x[2 * i + 1] - __uint_as_float(hb[i] & 0xffff0000u);
    }
    l = cvt8<bf16>(r);
}

template <int FBM>
__global__ __launch_bounds__(256, 2) void aid_gemm_f32x3_kernel(const GemmGroup g) {
    typedef F32Tile<FBM> Tile;
    constexpr int NB = Tile::NB, RS = Tile::RS;
    constexpr int PLANE = FBM * XLD, BUF = 4 * PLANE;                         // bf16 per plane and per buffer
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* const smem = reinterpret_cast<bf16*>(smem_raw);                     // [2 buffers][Ah, Al, Bh, Bl][rows][XLD]
    const Tile t(g);
    const GemmDesc& P = t.P;
    const int sq = (threadIdx.x & 3) * 8;                  // staging: a thread's k chunk of 8
    const float* ap[RS];
    const float* bp[RS];
    t.rows(P.a, P.stride_a, P.lda, P.b, P.stride_b, P.ldb, sq, ap, bp);
    typename Tile::Acc acc;
    Tile::zero(acc);

    f32x4 ra[RS][2], rb[RS][2];
    auto load = [&](int k0) {                              // k is a multiple of 8 (aid_hip.h): a chunk is inside the row or past it
        const bool in = k0 + sq < P.k;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < RS; ++i)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                ra[i][u] = in ? *reinterpret_cast<const f32x4*>(ap[i] + k0 + 4 * u) : z;
                rb[i][u] = in ? *reinterpret_cast<const f32x4*>(bp[i] + k0 + 4 * u) : z;
            }
    };
    auto store = [&](int buf) {                            // split on the way into LDS
        bf16* Ah = smem + buf * BUF;
        bf16* Bh = Ah + 2 * PLANE;
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const int o = (t.srow + 64 * i) * XLD + sq;
            bf16x8 h, l;
            split8(ra[i][0], ra[i][1], h, l);
            *reinterpret_cast<bf16x8*>(Ah + o) = h;
            *reinterpret_cast<bf16x8*>(Ah + PLANE + o) = l;
            split8(rb[i][0], rb[i][1], h, l);
            *reinterpret_cast<bf16x8*>(Bh + o) = h;
            *reinterpret_cast<bf16x8*>(Bh + PLANE + o) = l;
        }
    };

    const int nk = (P.k + XBK - 1) / XBK;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load((kt + 1) * XBK);
        const bf16* Ah = smem + (kt & 1) * BUF;
        const bf16* Bh = Ah + 2 * PLANE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {                   // two k-steps of 16 per tile
            bf16x8 fah[NB], fal[NB], fbh[NB], fbl[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int oa = (t.wm + 32 * i + t.l31) * XLD + 16 * ks + 8 * t.hi;
                const int ob = (t.wn + 32 * i + t.l31) * XLD + 16 * ks + 8 * t.hi;
                fah[i] = *reinterpret_cast<const bf16x8*>(Ah + oa);
                fal[i] = *reinterpret_cast<const bf16x8*>(Ah + PLANE + oa);
                fbh[i] = *reinterpret_cast<const bf16x8*>(Bh + ob);
                fbl[i] = *reinterpret_cast<const bf16x8*>(Bh + PLANE + ob);
            }
            // D[n][m]: lane (m = l31, hi) ends up with n = 8 g + 4 hi + e.  Term-outer: consecutive MFMAs go to different accumulators
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = mfma32(fbl[i], fah[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = mfma32(fbh[i], fal[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = mfma32(fbh[i], fah[j], acc[i][j]);
        }
        if (kt + 1 < nk) store((kt + 1) & 1);
        __syncthreads();
    }
    t.template epilogue<false>(acc, NoLR{});               // plain groups only (aid_abi.hip): no folded LayerNorm, no gain
}

template <int FBM>
constexpr size_t f32x3_lds_bytes() { return (size_t)2 * 4 * FBM * XLD * sizeof(bf16); }

hipError_t gemm_f32x3_launch(GemmGroup& g, hipStream_t stream) {
    static PerDevice<int> lds_set;
    int tiles;
    bool big;
    hipError_t e = gemm_f32_tiles(g, &tiles, &big);
    if (e != hipSuccess || tiles <= 0) return e;
    if (big) {
        e = set_max_dynamic_lds(lds_set, 0, reinterpret_cast<const void*>(&aid_gemm_f32x3_kernel<128>), f32x3_lds_bytes<128>());
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((aid_gemm_f32x3_kernel<128>), dim3(tiles), dim3(256), f32x3_lds_bytes<128>(), stream, g);
    } else {
        hipLaunchKernelGGL((aid_gemm_f32x3_kernel<64>), dim3(tiles), dim3(256), f32x3_lds_bytes<64>(), stream, g);
    }
    return hipGetLastError();
}

}  // namespace aid
