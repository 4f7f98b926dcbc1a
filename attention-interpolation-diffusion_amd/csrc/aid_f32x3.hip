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
//   aid_attn_f32x3_kernel   the float32 attention core (aid_attn_f32_kernel, aid_f32.hip) with K Q'^T and V^T P^T from the same split
//                           (AidAttnArgs.f32_split = 1); below the GEMM  [interpolation.py:626-664, 760-790]
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

// ------------------------------------------------------------------------------------------------
// attention core at "high" (AidAttnArgs.f32_split = 1): aid_attn_f32_kernel's pass structure (aid_f32.hip: 128 query rows per workgroup,
// 32 per wave, a lane owns one query row; 32-key tiles through LDS; online softmax with a running reference; TWO = OUTER's second
// accumulator set) with both products formed from bf16 halves.  The frame / head / query-block decode, the per-mode choice of segments
// and the output store are a second copy of that kernel's (sharing them would have changed its code).
//   * S^T = K Q'^T: Q' = Q c2 is split once per workgroup into registers — per 16-channel step g a lane (query l31, half hi) holds
//     channels 16 g + 8 hi .. + 7 as 4 + 4 packed VGPRs (D16 / 2 registers, what `qf` takes in the exact kernel).  K is split on the way
//     from the staging registers into two LDS planes of rows [32][D16 + 8] bf16 (D16 = channels padded to a multiple of 16 with zero
//     chunks, d = 40 -> 48): (D16 + 8) / 8 is odd, so the 16-byte fragment reads and staging writes are conflict-free.
//   * key order: key kk of a tile is stored in K row swap23(kk) (bits 2 and 3 exchanged, §3.1's trick).  Score register r of lane half
//     hi (result row (r & 3) + 8 (r >> 2) + 4 hi) is then key (r & 7) + 8 hi + 16 (r >> 3): registers 0 .. 7 are, as they lie, the B
//     operand of key step 0 .. 15 and registers 8 .. 15 that of key step 16 .. 31 — P needs no cross-lane movement and the V^T tile keeps
//     its keys in natural order (with the K rows swapped, swapping the V^T columns too would undo it).
//   * softmax: fp32 and unrounded (exp2f, running reference, alpha rescale); the row sum comes from the fp32 P.
//   * O^T += V^T P^T: P is split in registers (16 fp32 -> 8 + 8 packed VGPRs; P <= 1 and bf16 keeps the fp32 exponent range, so small
//     probabilities keep their low half); V^T is split on the way into two LDS planes of rows [DP][32 + 8] bf16.  Terms Vl Ph, Vh Pl,
//     Vh Ph; Vl Pl is dropped like the GEMM's fourth term.
//   * staging as in the exact kernel: global fp32 16-byte loads into registers; d <= 80: the next tile in flight across the arithmetic,
//     two LDS buffers, one barrier per tile; d = 160 single-buffered.
// ------------------------------------------------------------------------------------------------
constexpr int XKT = 32;                    // keys per tile

struct AttnF32x3Params {
    AidAttnArgs a;
    float c2;                              // softmax_scale * log2(e)  (1 when q is pre-scaled)
};

// key of score register r in lane half hi, with the K rows stored bits 2 <-> 3 swapped
__device__ __forceinline__ int key_of_x3(int r, int hi) { return (r & 7) + 8 * hi + 16 * (r >> 3); }
__device__ __forceinline__ int swap23(int kk) { return (kk & ~12) | ((kk & 4) << 1) | ((kk & 8) >> 1); }

template <int D, bool TWO>
__global__ __launch_bounds__(256, (D == 40 ? 2 : D == 64 ? 2 : D == 80 ? (TWO ? 1 : 2) : 1)) void aid_attn_f32x3_kernel(const AttnF32x3Params p) {
    constexpr int D16 = (D + 15) / 16 * 16, NS = D16 / 16;         // channels padded to whole 16-deep k-steps of the score product
    constexpr int DP = (D + 31) / 32 * 32, NDB = DP / 32;          // ... and to whole 32-blocks of the PV product
    constexpr int KLD = D16 + 8;                                   // K planes: rows [32][D16 + 8] bf16
    constexpr int VLD = XKT + 8;                                   // V^T planes: rows [DP][40] bf16
    static_assert((KLD / 8) % 2 == 1 && (VLD / 8) % 2 == 1 && D % 8 == 0, "conflict-free 16-byte fragment reads");
    constexpr bool PF = D <= 80;
    constexpr int NBUF = PF ? 2 : 1;
    constexpr int KC8 = D16 / 8;                                   // 8-channel chunks per key (pad chunks included)
    constexpr int KCH = XKT * KC8, VCH = DP * (XKT / 8);           // 8-element chunks of a K / V^T tile
    constexpr int NKC = (KCH + 255) / 256, NVC = (VCH + 255) / 256;
    constexpr int KPL = XKT * KLD, VPL = DP * VLD;                 // bf16 per plane
    __shared__ __attribute__((aligned(16))) bf16 Ks_[NBUF * 2 * KPL];          // [buffer][high, low][row][KLD]
    __shared__ __attribute__((aligned(16))) bf16 Vs_[NBUF * 2 * VPL];
    const AidAttnArgs& a = p.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int nqb = (a.s + 127) / 128;
    int bid = blockIdx.x;
    const int qb = bid % nqb; bid /= nqb;
    const int h = bid % a.heads;
    const int fr = bid / a.heads;
    const int q = qb * 128 + wave * 32 + l31;                       // this lane's query row (both lane halves share it)
    const bool qok = q < a.s;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

    const float* __restrict__ Q = reinterpret_cast<const float*>(a.q) + (int64_t)fr * a.q_fs + (int64_t)min(q, a.s - 1) * a.ldq + h * D;
    // Q' = Q softmax_scale log2(e), split: step g of lane (l31, hi) holds channels 16 g + 8 hi .. + 7 (pad channels: zero)
    bf16x8 qh[NS], ql[NS];
#pragma unroll
    for (int g = 0; g < NS; ++g) {
        const int c0 = 16 * g + 8 * hi;
        f32x4 x0 = z4, x1 = z4;
        if (D % 16 == 0 || c0 < D) {
            x0 = *reinterpret_cast<const f32x4*>(Q + c0) * p.c2;
            x1 = *reinterpret_cast<const f32x4*>(Q + c0 + 4) * p.c2;
        }
        split8(x0, x1, qh[g], ql[g]);
    }

    // ---- what this frame attends with (decided per frame from the coefficient, like aid_attn_f32_kernel)
    const float cf = (a.mode != AID_MODE_PLAIN && a.coef) ? a.coef[fr] : -1.f;
    const bool plain = a.mode == AID_MODE_PLAIN || cf < 0.f;       // a negative coefficient marks a PLAIN rider
    const int own = a.kv_map ? a.kv_map[fr] : fr;
    const float* const K0 = reinterpret_cast<const float*>(a.k);
    const float* const V0 = reinterpret_cast<const float*>(a.vt);

    // additive score bias: the row of this lane's query; element j goes with key j of every segment
    const float* const brow = a.bias ? reinterpret_cast<const float*>(a.bias) + (int64_t)fr * a.bias_fs + (int64_t)h * a.bias_hs +
                                           (int64_t)min(q, a.s - 1) * a.bias_rs
                                     : nullptr;

    f32x16 res[NDB];                                               // sum over passes of weight * O^T
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) res[d][r] = 0.f;

    // one softmax pass over up to two key segments; its normalised output is added to `res` with weight w
    auto pass = [&](const float* k1, const float* v1, const float* k2, const float* v2, float w) {
        f32x16 otmp[NDB];
        f32x16 (&o)[NDB] = TWO ? otmp : res;                        // one pass per frame: accumulate where the result lives
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
        float mrow = -INFINITY, lsum = 0.f;                         // running reference and this lane half's partial row sum
        float bref = -1e30f;                                        // score bias: its largest (clamped) value of the row so far
        const int ntl = (a.l + XKT - 1) / XKT;                      // tiles per segment
        const int nt = (k2 ? 2 : 1) * ntl;                          // (k1 is never null)
        f32x4 rk[NKC][2], rv[NVC][2];
        // tile i of the pass -> registers, 8 channels of a key / 8 keys of a channel per chunk (past the tile / the keys / the
        // channels: zero)
        auto gload = [&](int i) {
            const float* kp = i >= ntl ? k2 : k1;
            const float* vp = i >= ntl ? v2 : v1;
            const int t0 = (i >= ntl ? i - ntl : i) * XKT;
#pragma unroll
            for (int u = 0; u < NKC; ++u) {                         // K tile [key][channel]
                const int id = tid + 256 * u;
                const int kk = id / KC8, c = (id - kk * KC8) * 8;
                const bool in = (KCH % 256 == 0 || id < KCH) && t0 + kk < a.l && (D % 16 == 0 || c < D);
                const float* src = kp + (int64_t)(t0 + kk) * a.ldk + h * D + c;
                rk[u][0] = in ? *reinterpret_cast<const f32x4*>(src) : z4;
                rk[u][1] = in ? *reinterpret_cast<const f32x4*>(src + 4) : z4;
            }
#pragma unroll
            for (int u = 0; u < NVC; ++u) {                         // V^T tile [channel][key]; keys past L and pad channels are zero
                const int id = tid + 256 * u;
                const int c = id / (XKT / 8), kk = (id - c * (XKT / 8)) * 8;
                const bool in = (VCH % 256 == 0 || id < VCH) && (D % 32 == 0 || c < D);
                const float* src = vp + (int64_t)(h * D + c) * a.ldvt + t0 + kk;
#pragma unroll
                for (int hq = 0; hq < 2; ++hq) {                    // (ldvt, t0 and kk are multiples of 4)
                    const int k0 = t0 + kk + 4 * hq;
                    f32x4 v = z4;
                    if (in && k0 < a.l) {
                        if (k0 + 3 < a.l) v = *reinterpret_cast<const f32x4*>(src + 4 * hq);
                        else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = (k0 + e < a.l) ? src[4 * hq + e] : 0.f;
                        }
                    }
                    rv[u][hq] = v;
                }
            }
        };
        auto lstore = [&](int buf) {                                // split on the way into LDS
            bf16* Kb = Ks_ + buf * 2 * KPL;
            bf16* Vb = Vs_ + buf * 2 * VPL;
#pragma unroll
            for (int u = 0; u < NKC; ++u) {
                const int id = tid + 256 * u;
                const int kk = id / KC8, c = (id - kk * KC8) * 8;
                if (KCH % 256 == 0 || id < KCH) {
                    bf16x8 xh, xl;
                    split8(rk[u][0], rk[u][1], xh, xl);
                    const int o8 = swap23(kk) * KLD + c;
                    *reinterpret_cast<bf16x8*>(Kb + o8) = xh;
                    *reinterpret_cast<bf16x8*>(Kb + KPL + o8) = xl;
                }
            }
#pragma unroll
            for (int u = 0; u < NVC; ++u) {
                const int id = tid + 256 * u;
                const int c = id / (XKT / 8), kk = (id - c * (XKT / 8)) * 8;
                if (VCH % 256 == 0 || id < VCH) {
                    bf16x8 xh, xl;
                    split8(rv[u][0], rv[u][1], xh, xl);
                    const int o8 = c * VLD + kk;
                    *reinterpret_cast<bf16x8*>(Vb + o8) = xh;
                    *reinterpret_cast<bf16x8*>(Vb + VPL + o8) = xl;
                }
            }
        };
        __syncthreads();                                            // the previous pass has been consumed by every wave
        if (PF) {
            gload(0);
            lstore(0);
            __syncthreads();
        }
        for (int it = 0; it < nt; ++it) {
            const int t0 = (it >= ntl ? it - ntl : it) * XKT;
            const bf16* Kh = Ks_ + (PF ? (it & 1) : 0) * 2 * KPL;
            const bf16* Vh = Vs_ + (PF ? (it & 1) : 0) * 2 * VPL;
            if (PF) {
                if (it + 1 < nt) gload(it + 1);                     // in flight across this tile's arithmetic
            } else {
                if (it) __syncthreads();                            // the previous tile has been consumed by every wave
                gload(it);
                lstore(0);
                __syncthreads();
            }
            if (brow) {                                            // the tile's largest bias per row, before the scores take their registers
                float bm = -1e30f;
#pragma unroll
                for (int r = 0; r < 16; ++r) bm = fmaxf(bm, brow[min(t0 + key_of_x3(r, hi), a.l - 1)]);
                asm volatile("" ::: "memory");                     // (the loads below are issued again: 16 values are not kept live)
                const float bnew = fmaxf(bref, max_halves(bm));
                mrow += (bref - bnew) * 1.4426950408889634f;       // (-inf stays -inf: both references are finite)
                bref = bnew;
            }
            // S^T = K Q'^T, low-order terms first: lane (query l31, half hi) receives the scores of keys key_of_x3(r, hi)
            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                const int o8 = l31 * KLD + 16 * g + 8 * hi;
                const bf16x8 kh = *reinterpret_cast<const bf16x8*>(Kh + o8);
                const bf16x8 kl = *reinterpret_cast<const bf16x8*>(Kh + KPL + o8);
                sc = mfma32(kl, qh[g], sc);
                sc = mfma32(kh, ql[g], sc);
                sc = mfma32(kh, qh[g], sc);
            }
            if (brow) {
                // scale q k^T + bias, in the log2 domain (values below -1e30 clamped), relative to the largest bias of the row so far
                // like in aid_attn_f32_kernel (aid_f32.hip); the cases are spelt out at the BIAS instantiation in aid_attn.hip
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float db = fmaxf(brow[min(t0 + key_of_x3(r, hi), a.l - 1)], -1e30f) - bref;
                    asm volatile("" : "+v"(db));                   // the difference first: -ffast-math may not spread it over the sum
                    sc[r] += db * 1.4426950408889634f;
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (t0 + key_of_x3(r, hi) >= a.l) sc[r] = -INFINITY;
                mx = fmaxf(mx, sc[r]);
            }
            mx = max_halves(mx);
            const float mnew = fmaxf(mrow, mx);                    // finite: every tile holds at least one key
            const float alpha = exp2f(mrow - mnew);                // 0 on the first tile (mrow = -inf)
            mrow = mnew;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[r] = exp2f(sc[r] - mnew);
                ps += sc[r];
            }
            lsum = lsum * alpha + ps;
            // P split in registers: registers 8 ks .. 8 ks + 7 are keys 16 ks + 8 hi + {0 .. 7}, the B operand of key step ks
            bf16x8 ph[2], pl[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f32x4 x0 = {sc[8 * ks], sc[8 * ks + 1], sc[8 * ks + 2], sc[8 * ks + 3]};
                const f32x4 x1 = {sc[8 * ks + 4], sc[8 * ks + 5], sc[8 * ks + 6], sc[8 * ks + 7]};
                split8(x0, x1, ph[ks], pl[ks]);
            }
            // O^T = alpha O^T + V^T P^T
            if (__any(alpha != 1.f)) {                              // (most tiles leave every row's reference where it was)
#pragma unroll
                for (int d = 0; d < NDB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 vh[NDB], vl[NDB];
#pragma unroll
                for (int d = 0; d < NDB; ++d) {
                    const int o8 = (32 * d + l31) * VLD + 16 * ks + 8 * hi;
                    vh[d] = *reinterpret_cast<const bf16x8*>(Vh + o8);
                    vl[d] = *reinterpret_cast<const bf16x8*>(Vh + VPL + o8);
                }
                // term-outer: consecutive MFMAs go to different accumulators
#pragma unroll
                for (int d = 0; d < NDB; ++d) o[d] = mfma32(vl[d], ph[ks], o[d]);
#pragma unroll
                for (int d = 0; d < NDB; ++d) o[d] = mfma32(vh[d], pl[ks], o[d]);
#pragma unroll
                for (int d = 0; d < NDB; ++d) o[d] = mfma32(vh[d], ph[ks], o[d]);
            }
            if (PF) {
                if (it + 1 < nt) lstore((it + 1) & 1);              // that buffer was last read a barrier ago
                __syncthreads();
            }
        }
        const float inv = w / sum_halves(lsum);
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) res[d][r] = TWO ? fmaf(o[d][r], inv, res[d][r]) : o[d][r] * inv;
    };

    const float* k_own = K0 + (int64_t)own * a.k_fs;
    const float* v_own = V0 + (int64_t)own * a.vt_fs;
    if (plain) {
        pass(k_own, v_own, nullptr, nullptr, 1.f);
    } else if (a.mode == AID_MODE_INNER) {
        // interpolated keys / values: k2 / vt2 row of the frame for 0 < c < 1, the end-point frames themselves for c = 0 / 1
        const float* km;
        const float* vm;
        if (cf > 0.f && cf < 1.f) {
            km = reinterpret_cast<const float*>(a.k2) + (int64_t)fr * a.k_fs;
            vm = reinterpret_cast<const float*>(a.vt2) + (int64_t)fr * a.vt_fs;
        } else {
            const int e = cf == 0.f ? a.begin : a.end;
            km = K0 + (int64_t)e * a.k_fs;
            vm = V0 + (int64_t)e * a.vt_fs;
        }
        if (a.fused) pass(k_own, v_own, km, vm, 1.f);
        else         pass(km, vm, nullptr, nullptr, 1.f);
    } else {                                                       // OUTER: (1 - c) A(.., begin) + c A(.., end); a zero weight drops its side
        const float* kb = K0 + (int64_t)a.begin * a.k_fs;
        const float* vb = V0 + (int64_t)a.begin * a.vt_fs;
        const float* ke = K0 + (int64_t)a.end * a.k_fs;
        const float* ve = V0 + (int64_t)a.end * a.vt_fs;
        if (cf != 1.f) { if (a.fused) pass(k_own, v_own, kb, vb, 1.f - cf); else pass(kb, vb, nullptr, nullptr, 1.f - cf); }
        if (cf != 0.f) { if (a.fused) pass(k_own, v_own, ke, ve, cf);       else pass(ke, ve, nullptr, nullptr, cf); }
    }

    // ---- out_i = (accumulate ? out_i : 0) + out_scale * frame_scale[i] * O_i; lane (q, hi) holds channels 32 d + 8 g + 4 hi + e
    if (!qok) return;
    const float osc = a.out_scale * (a.frame_scale ? a.frame_scale[fr] : 1.f);
    float* orow = reinterpret_cast<float*>(a.out) + (int64_t)fr * a.o_fs + (int64_t)q * a.ldo + h * D;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int dv = 32 * d + 8 * gq + 4 * hi + e;
                if (dv < D) {
                    float v = res[d][4 * gq + e] * osc;
                    if (a.accumulate) v += orow[dv];
                    orow[dv] = v;
                }
            }
}

template <int D>
static hipError_t attn_f32x3_run(const AttnF32x3Params& p, hipStream_t stream) {
    const int nqb = (p.a.s + 127) / 128;
    if (p.a.mode == AID_MODE_OUTER)
        hipLaunchKernelGGL((aid_attn_f32x3_kernel<D, true>), dim3(nqb * p.a.heads * p.a.n_frames), dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL((aid_attn_f32x3_kernel<D, false>), dim3(nqb * p.a.heads * p.a.n_frames), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// what plan_attn may put on the split kernel (AidAttnArgs.f32_split is a permission): every head dim and mode the exact kernel runs
bool attn_f32x3_supported(const AidAttnArgs& a) {
    return a.dtype == AID_DTYPE_F32 && (a.d == 40 || a.d == 64 || a.d == 80 || a.d == 160);
}

hipError_t attn_f32x3_launch(const AidAttnArgs& a, hipStream_t stream) {
    AttnF32x3Params p;
    p.a = a;
    p.c2 = a.q_prescaled ? 1.f : a.softmax_scale * 1.4426950408889634f;
    switch (a.d) {
        case 40:  return attn_f32x3_run<40>(p, stream);
        case 64:  return attn_f32x3_run<64>(p, stream);
        case 80:  return attn_f32x3_run<80>(p, stream);
        case 160: return attn_f32x3_run<160>(p, stream);
        default:  return hipErrorInvalidValue;
    }
}

}  // namespace aid
