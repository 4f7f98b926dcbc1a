// Does the MFMA SHAPE change the clock this box holds under a dense matrix load?
// tools/ubench/mfma_ceiling.hip shows that on random operands the chip is power-bound: the clock, not the issue rate, sets the
// FLOP/s.  This program runs the same products as v_mfma_f32_32x32x16 and as v_mfma_f32_16x16x32 (half the flops per instruction,
// half the cycles: equal cycles per flop) and reports what each sustains.  Every CU runs four waves (one per SIMD); a trip of
// either shape does the same flops on the same output tile with the same operand bytes.
//   reg  operands in registers: 128 x 64 x 64 per trip and wave — 32 MFMAs of 32x32x16 on 8 accumulators, or 64 of 16x16x32 on 32
//        (16 A + 8 B fragments of 16 bytes per lane either way).
//   lds  operands re-read every phase by ds_read_b128 from a static LDS image in the 288-row GEMM engine's layout (rows of 128 B,
//        16-byte chunk c of row r at slot c ^ ((r >> 1) & 7)) at the engine's ratio: 16 reads per phase of 16 MFMAs of 32x32x16
//        (64 x 64 x 64: 2 x 2 blocks, 4 k-steps) or of 32 MFMAs of 16x16x32 (4 x 4 blocks, 2 k-steps); two phases per trip, the
//        reads of a phase issued ahead of the previous phase's MFMAs.  32x32x16: lane reads row l & 31, chunks 2 ks + (l >> 5);
//        16x16x32: row l & 15, chunks 4 j + (l >> 4).  Both are conflict-free under the ds_read_b128 lane groups.
//   attn the ping-pong attention kernel's mix: eight waves per CU in two groups one barrier apart, an M slot of one group against the
//        V slot (exponentials, conversions) of the other on every SIMD — described at k_attn below.
// Operand sets as in mfma_ceiling: zeros, N(0, 1) samples rounded to bf16, N(0, 1) samples rounded to f16.
// Per cell: TFLOP/s (wall), wave cycles per 32768 flop (= per 32x32x16 MFMA; 32 is the pipe's floor), effective GHz = cycles / wall.
// The sweep runs twice so the spread between two runs of one cell can be set against the difference between the shapes.
// build: hipcc --offload-arch=gfx950 -O3 -o mfma_shape mfma_shape.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include <algorithm>
#include <type_traits>
typedef _Float16 f16;
typedef __bf16 bf16;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef bf16 b8 __attribute__((ext_vector_type(8)));
typedef f16 h8 __attribute__((ext_vector_type(8)));

template <bool BF>
__device__ __forceinline__ f32x16 mma32(u16x8 a, u16x8 b, f32x16 c) {
    if (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
    else    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}
template <bool BF>
__device__ __forceinline__ f32x4 mma16(u16x8 a, u16x8 b, f32x4 c) {
    if (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
    else    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// ---- operands in registers ------------------------------------------------------------------------------------------------
template <int SH, bool BF>
__global__ __launch_bounds__(256) void k_reg(const unsigned short* __restrict__ src, float* out, long long* cyc, int iters) {
    u16x8 fr[24];                                                             // 16 A, 8 B
    const unsigned short* p = src + ((size_t)blockIdx.x * 256 + threadIdx.x) * 256;
#pragma unroll
    for (int i = 0; i < 24; ++i) fr[i] = *reinterpret_cast<const u16x8*>(p + 8 * i);
    constexpr int NA = SH == 32 ? 8 : 32, NR = SH == 32 ? 16 : 4;
    typedef typename std::conditional<SH == 32, f32x16, f32x4>::type ACC;
    ACC acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[j][r] = 0.f;
    __syncthreads();
    const long long c0 = clock64();
    for (int it = 0; it < iters; ++it) {
        if constexpr (SH == 32) {
#pragma unroll
            for (int g = 0; g < 32; ++g) {                                    // 4 k-steps x (4 x 2 blocks of 32 x 32)
                const int ks = g >> 3, i = g & 3, j = (g >> 2) & 1;
                acc[g & 7] = mma32<BF>(fr[16 + 4 * j + ks], fr[4 * i + ks], acc[g & 7]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int g = 0; g < 64; ++g) {                                    // 2 k-steps x (8 x 4 blocks of 16 x 16)
                const int ks = g >> 5, i = g & 7, j = (g >> 3) & 3;
                acc[g & 31] = mma16<BF>(fr[16 + 2 * j + ks], fr[2 * i + ks], acc[g & 31]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const long long c1 = clock64();
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int r = 0; r < NR; ++r) s += acc[j][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = c1 - c0;
}

// ---- operands from LDS ------------------------------------------------------------------------------------------------------
// LDS image: 256 A rows then 256 B rows of 128 B (64 KB).  Wave w, phase p: A rows 128 (w & 1) + 64 p .. + 63, B rows
// 64 (w >> 1) + 128 p .. + 63.  The data is random, so the swizzle only has to be honoured by the reads.  One read follows each
// MFMA of 32x32x16 (every second one of 16x16x32), in that order in the binary (sched_barrier).
template <int SH, bool BF>
__global__ __launch_bounds__(256) void k_lds(const unsigned short* __restrict__ src, float* out, long long* cyc, int iters) {
    __shared__ __attribute__((aligned(16))) char img[65536];
    const unsigned short* p = src + (size_t)blockIdx.x * 65536;               // 32768 of the block's 65536 values fill the image
#pragma unroll
    for (int i = 0; i < 16; ++i)
        *reinterpret_cast<u16x8*>(img + (threadIdx.x + 256 * i) * 16) = *reinterpret_cast<const u16x8*>(p + (threadIdx.x + 256 * i) * 8);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NK = SH == 32 ? 4 : 2;                                      // fragments along k of one block row
    constexpr int NA = SH == 32 ? 4 : 16, NR = SH == 32 ? 16 : 4;             // accumulators of a phase, registers of one
    constexpr int NM = SH == 32 ? 16 : 32;                                    // MFMAs of a phase
    typedef typename std::conditional<SH == 32, f32x16, f32x4>::type ACC;
    ACC acc[2][NA];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[q][j][r] = 0.f;
    // byte offset of this lane's chunk c in block row 0 of phase 0, A and B
    int la[NK], lb[NK];
    {
        const int r = lane & (SH - 1), kq = lane / SH, sw = (r >> 1) & 7;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const int chunk = ((SH == 32 ? 2 * c : 4 * c) + kq) ^ sw;
            la[c] = (128 * (w & 1) + r) * 128 + chunk * 16;
            lb[c] = (256 + 64 * (w >> 1) + r) * 128 + chunk * 16;
        }
    }
    // read i (0 .. 15) of phase ph: 0 - 7 the B fragments, 8 - 15 the A fragments; fragment index = block row * NK + chunk
    auto rd = [&](int ph, int i) __attribute__((always_inline)) {
        const int idx = i & 7, e = idx / NK, c = idx % NK;
        const int off = i < 8 ? lb[c] + (e * SH + 128 * ph) * 128 : la[c] + (e * SH + 64 * ph) * 128;
        return *reinterpret_cast<const u16x8*>(img + off);
    };
    __syncthreads();
    u16x8 fa[2][8], fb[2][8];
#pragma unroll
    for (int i = 0; i < 16; ++i) (i < 8 ? fb : fa)[0][i & 7] = rd(0, i);
    const long long c0 = clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < NK; ++c) {                                        // the image is static: keep the reads inside the loop
            asm volatile("" : "+v"(la[c]));
            asm volatile("" : "+v"(lb[c]));
        }
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                if constexpr (SH == 32) {
                    const int ks = i >> 2, in = (i >> 1) & 1, e = i & 1;
                    acc[ph][2 * in + e] = mma32<BF>(fb[ph][in * 4 + ks], fa[ph][e * 4 + ks], acc[ph][2 * in + e]);
                    (i < 8 ? fb : fa)[ph ^ 1][i & 7] = rd(ph ^ 1, i);         // the next phase's fragments, under this phase's MFMAs
                } else {
                    const int j = i >> 4, in = (i >> 2) & 3, e = i & 3;
                    acc[ph][4 * in + e] = mma16<BF>(fb[ph][in * 2 + j], fa[ph][e * 2 + j], acc[ph][4 * in + e]);
                    if (i & 1) (i < 16 ? fb : fa)[ph ^ 1][(i >> 1) & 7] = rd(ph ^ 1, i >> 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const long long c1 = clock64();
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) s += acc[q][j][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + w] = c1 - c0;
}

// ---- the ping-pong attention kernel's mix -------------------------------------------------------------------------------------
// Workgroups of 8 waves, one per CU; waves w and w + 4 share a SIMD and run the same program ONE BARRIER APART (csrc/aid_attn_pp.hip):
// per 64-key tile an M slot — every MFMA of the tile, the 16 fragment reads in their shadow in pinned order, no VALU — and a V slot —
// P = 2^S rounded to the storage type: 32 v_exp_f32, 16 packed conversions, bf16: the OR chain of the head-room test, f16: the
// v_dot2c row sum — so one wave of a SIMD runs matrix instructions while its partner runs the exponentials.  A wave owns 32 query rows.
//   32x32x16  S^T = K Q'^T - m: 2 key blocks x 4 k-steps = 8 MFMAs, O^T += V^T P^T: 2 channel blocks x 4 k-steps = 8; bf16: + eight
//             4x4x4 row-sum MFMAs behind the PV MFMAs (as the kernel).  Reads: lane row l & 31 (K: key bits 2 <-> 3 swapped), chunk
//             2 ks + (l >> 5).
//   16x16x32  the same flops as 4 key blocks x 2 row blocks x 2 k-steps = 32 + 4 channel blocks x 2 row blocks x 2 k-steps = 32, every
//             block's first k-step before any second; bf16: + four row-sum MFMAs with a ones A operand (64 cycles, like the eight
//             4x4x4).  Reads: the same 16, one beside every second MFMA; lane row l & 15 of the block (K: row
//             32 (kb >> 1) + 8 ((l & 15) >> 2) + 4 ((l >> 1) & 1) + 2 (kb & 1) + (l & 1), so that a lane's eight P values of a k-step
//             are eight consecutive keys and the reads are conflict-free), chunk 4 ks + (l >> 4).
// LDS: a static image of four ring stages (K tile at 8 KB x stage, V^T tile at 32 KB + 8 KB x stage), rows of 128 B, 16-byte chunk c of
// row r at slot c ^ ((r >> 1) & 7); the stage is a constant in each of four unrolled copies.  No DMA: the image does not change.
// Q' is the block's N(0, 1) data / 8 (the softmax scale of d = 64), so the scores are N(0, 1) and P = 2^(S - 8) stays in range.
template <bool BF>
__device__ __forceinline__ u16x8 pack8(const float* x) {
    u16x8 r;
    if (BF) {
        typedef bf16 b2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 v; v[0] = x[2 * i]; v[1] = x[2 * i + 1];
            const b2 c = __builtin_convertvector(v, b2);
            const unsigned int w = __builtin_bit_cast(unsigned int, c);
            r[2 * i] = (unsigned short)w; r[2 * i + 1] = (unsigned short)(w >> 16);
        }
    } else {
        typedef f16 h2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 v; v[0] = x[2 * i]; v[1] = x[2 * i + 1];
            const h2 c = __builtin_convertvector(v, h2);
            const unsigned int w = __builtin_bit_cast(unsigned int, c);
            r[2 * i] = (unsigned short)w; r[2 * i + 1] = (unsigned short)(w >> 16);
        }
    }
    return r;
}
template <bool BF>
__device__ __forceinline__ u16x8 eighth(u16x8 v) {                            // v / 8, exact
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (BF) x[i] = __uint_as_float((unsigned int)v[i] << 16) * 0.125f;
        else { f16 h; unsigned short s = v[i]; __builtin_memcpy(&h, &s, 2); x[i] = (float)h * 0.125f; }
    }
    return pack8<BF>(x);
}

template <int SH, bool BF>
__global__ __launch_bounds__(512) void k_attn(const unsigned short* __restrict__ src, float* out, long long* cyc, int iters) {
    __shared__ __attribute__((aligned(16))) char img[65536];
    const unsigned short* p = src + (size_t)blockIdx.x * 65536;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        *reinterpret_cast<u16x8*>(img + (threadIdx.x + 512 * i) * 16) = *reinterpret_cast<const u16x8*>(p + (threadIdx.x + 512 * i) * 8);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = w >> 2;
    constexpr int VB = 32768, ST = 8192;
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    u16x8 qf[4], kf[8], vf[8], pf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qf[i] = eighth<BF>(*reinterpret_cast<const u16x8*>(p + 32768 + (threadIdx.x * 4 + i) * 8));
        pf[i] = qf[i];
    }
    constexpr int NR = SH == 32 ? 16 : 4, NB = 32 / NR;                       // registers of an accumulator block, blocks of S and of O
    typedef typename std::conditional<SH == 32, f32x16, f32x4>::type ACC;
    ACC S[NB], O[NB];                                                         // 16x16x32: S[2 kb + rb], O[2 cb + rb]
#pragma unroll
    for (int i = 0; i < 32; ++i) { S[i / NR][i % NR] = -8.f; O[i / NR][i % NR] = 0.f; }
    float cneg = -8.f;
    asm volatile("" : "+v"(cneg));
    f32x4 lacc = {0.f, 0.f, 0.f, 0.f}, lrs[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    s16x4 ones4;
    u16x8 ones8;
#pragma unroll
    for (int i = 0; i < 4; ++i) ones4[i] = 0x3f80;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones8[i] = 0x3f80;
    asm volatile("" : "+v"(ones4));
    asm volatile("" : "+v"(ones8));
    float lsum = 0.f;
    unsigned int flag = 0;

    // per-lane byte offsets of the fragments: index i = 0 .. 7 -> register kad[i & 3] / vad[...] + a constant
    int kad[4], vad[4];
    if constexpr (SH == 32) {
        const int l31 = lane & 31, hi = lane >> 5;
        const int krow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
        const int kx = hi ^ ((krow >> 1) & 7), vx = hi ^ ((l31 >> 1) & 7);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kad[ks] = krow * 128 + (((2 * ks) ^ kx) << 4);
            vad[ks] = VB + l31 * 128 + (((2 * ks) ^ vx) << 4);
        }
    } else {
        const int l15 = lane & 15, g = lane >> 4;
        const int kb0 = 8 * (l15 >> 2) + 4 * ((l15 >> 1) & 1) + (l15 & 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int row = kb0 + 2 * b;
                kad[2 * ks + b] = row * 128 + (((4 * ks + g) ^ ((row >> 1) & 7)) << 4);
            }
            vad[ks] = VB + l15 * 128 + (((4 * ks + g) ^ ((l15 >> 1) & 7)) << 4);
            vad[2 + ks] = 0;
        }
    }
    // fragment i of a tile.  32x32x16: i = 2 ks + block.  16x16x32: K i = 4 ks + key block, V^T i = 4 ks + channel block
    auto rk = [&](int st, int i) __attribute__((always_inline)) {
        const int off = SH == 32 ? kad[i >> 1] + (i & 1) * 4096 : kad[2 * (i >> 2) + (i & 1)] + ((i >> 1) & 1) * 4096;
        return *reinterpret_cast<const u16x8*>(img + off + st * ST);
    };
    auto rv = [&](int st, int i) __attribute__((always_inline)) {
        const int off = SH == 32 ? vad[i >> 1] + (i & 1) * 4096 : vad[i >> 2] + (i & 3) * 2048;
        return *reinterpret_cast<const u16x8*>(img + off + st * ST);
    };
    auto pin = []() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };
    auto bar = [&]() __attribute__((always_inline)) { pin(); __builtin_amdgcn_s_barrier(); pin(); };

    auto mslot = [&](int sv, int sk) __attribute__((always_inline)) {
        pin();
        if constexpr (SH == 32) {
            f32x16 c16;
#pragma unroll
            for (int r = 0; r < 16; ++r) c16[r] = cneg;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ks = i >> 1, b = i & 1;
                vf[i] = rv(sv, i);
                pin();
                S[b] = mma32<BF>(kf[i], qf[ks], ks ? S[b] : c16);
                pin();
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kk = i >> 1, b = i & 1;
                O[b] = mma32<BF>(vf[i], pf[kk], O[b]);
                pin();
                if constexpr (BF) {
                    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
                    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
                    const u4 w4 = __builtin_bit_cast(u4, pf[kk]);
                    u2 h2; h2[0] = w4[2 * b]; h2[1] = w4[2 * b + 1];
                    lacc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones4, __builtin_bit_cast(s16x4, h2), lacc, 0, 0, 0);
                    pin();
                }
                kf[i] = rk(sk, i);
                pin();
            }
        } else {
            f32x4 c4 = {cneg, cneg, cneg, cneg};
#pragma unroll
            for (int i = 0; i < 16; ++i) {                                    // i = 8 ks + 2 kb + rb
                const int ks = i >> 3, kb = (i >> 1) & 3, rb = i & 1;
                if (i & 1) { vf[i >> 1] = rv(sv, i >> 1); pin(); }
                S[2 * kb + rb] = mma16<BF>(kf[4 * ks + kb], qf[2 * rb + ks], ks ? S[2 * kb + rb] : c4);
                pin();
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {                                    // i = 8 ks + 2 cb + rb
                const int ks = i >> 3, cb = (i >> 1) & 3, rb = i & 1;
                O[2 * cb + rb] = mma16<BF>(vf[4 * ks + cb], pf[2 * rb + ks], O[2 * cb + rb]);
                pin();
                if constexpr (BF) {
                    if ((i & 3) == 3) {                                       // the four row-sum MFMAs: (row block, k-step) = i >> 2
                        const int j = i >> 2;
                        lrs[j & 1] = mma16<true>(ones8, pf[2 * (j & 1) + (j >> 1)], lrs[j & 1]);
                        pin();
                    }
                }
                if (i & 1) { kf[i >> 1] = rk(sk, i >> 1); pin(); }
            }
        }
    };
    auto vslot = [&]() __attribute__((always_inline)) {
        unsigned int acc = 0;
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float pv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // 32x32x16: fragment f = 2 b + u holds sc[b][8 u + e]; 16x16x32: f = 2 rb + ks holds S[2 (2 ks + ((e >> 1) & 1)) + rb][(e & 1) + 2 (e >> 2)]
                const int idx = SH == 32 ? 8 * f + e : 4 * (2 * (2 * (f & 1) + ((e >> 1) & 1)) + (f >> 1)) + (e & 1) + 2 * (e >> 2);
                pv[e] = __builtin_amdgcn_exp2f(S[idx / NR][idx % NR]);
            }
            pf[f] = pack8<BF>(pv);
            typedef unsigned int u4 __attribute__((ext_vector_type(4)));
            const u4 w4 = __builtin_bit_cast(u4, pf[f]);
            if constexpr (BF) {
                acc = f == 0 ? (w4[0] | w4[1] | w4[2]) | w4[3] : (acc | w4[0] | w4[1]) | (w4[2] | w4[3]);
            } else {
                typedef f16 h2 __attribute__((ext_vector_type(2)));
                h2 one; one[0] = (f16)1.0f; one[1] = (f16)1.0f;
                t0 = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w4[0]), one, t0, false);
                t1 = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w4[1]), one, t1, false);
                t0 = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w4[2]), one, t0, false);
                t1 = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w4[3]), one, t1, false);
            }
        }
        if constexpr (BF) {
            if (__builtin_expect(__any((acc & 0x40004000u) != 0u), 0)) flag += 1;       // the head-room test; never taken on these operands
        } else {
            const float ts = t0 + t1;
            if (__builtin_expect(__any(ts > 32768.f), 0)) flag += 1;
            lsum += ts;
        }
    };

    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) kf[i] = rk(0, i);
    if (grp == 1) bar();                                                      // the second group runs one barrier behind
    const long long c0 = clock64();
    for (int it = 0; it < iters; it += 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                         // the image is static: keep the reads inside the loop
            asm volatile("" : "+v"(kad[c]));
            asm volatile("" : "+v"(vad[c]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            vslot();
            bar();
            mslot(i, (i + 2) & 3);
            bar();
        }
    }
    const long long c1 = clock64();
    if (grp == 0) bar();
    float s = lsum + (float)flag + lacc[0] + lrs[0][0] + lrs[1][1];
#pragma unroll
    for (int i = 0; i < 32; ++i) s += O[i / NR][i % NR] + S[i / NR][i % NR];
    out[blockIdx.x * 512 + threadIdx.x] = s;
    if (lane == 0) cyc[blockIdx.x * 8 + w] = c1 - c0;
}

struct Res { double tflops, ghz, cyc; };
typedef void (*Kern)(const unsigned short*, float*, long long*, int);

// `units` = 32768-flop units (one 32x32x16 MFMA's worth) per trip and wave; `nw` = waves per workgroup (one workgroup per CU)
Res run(Kern kern, const unsigned short* data, float* out, long long* cyc, int ncu, int iters, int units, int nw = 4) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    std::vector<float> ms;
    for (int it = 0; it < 7; ++it) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(ncu), dim3(64 * nw), 0, 0, data, out, cyc, iters);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float t; hipEventElapsedTime(&t, e0, e1);
        if (it >= 2) ms.push_back(t);                                         // two launches let the clock settle
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    std::vector<long long> hc(ncu * nw);
    hipMemcpy(hc.data(), cyc, hc.size() * sizeof(long long), hipMemcpyDeviceToHost);
    double cs = 0; for (auto c : hc) cs += (double)c;
    cs /= hc.size();
    hipEventDestroy(e0); hipEventDestroy(e1);
    const double u = (double)iters * units;
    Res r;
    r.tflops = u * nw * ncu * 32768.0 / (med * 1e-3) / 1e12;
    r.cyc = cs / u;
    r.ghz = cs / (med * 1e-3) * 1e-9;
    return r;
}

int main() {
    int dev = 0, ncu = 256;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const size_t n = (size_t)ncu * 256 * 256;
    std::vector<unsigned short> h(n);
    unsigned long long x = 88172645463325252ull;
    unsigned short *d_rand_bf, *d_rand_h, *d_zero;
    float* out; long long* cyc;
    hipMalloc(&d_rand_bf, n * 2); hipMalloc(&d_rand_h, n * 2); hipMalloc(&d_zero, n * 2);
    hipMalloc(&out, (size_t)ncu * 512 * 4); hipMalloc(&cyc, (size_t)ncu * 8 * sizeof(long long));
    auto uni = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return ((x >> 11) + 1) * (1.0 / 9007199254740993.0); };
    auto gauss = [&]() { const double u = uni(), v = uni(); return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v); };
    for (size_t i = 0; i < n; ++i) {
        const float g = (float)gauss();
        unsigned int b; memcpy(&b, &g, 4);
        b += 0x7fff + ((b >> 16) & 1);                                        // round to nearest even
        h[i] = (unsigned short)(b >> 16);
    }
    hipMemcpy(d_rand_bf, h.data(), n * 2, hipMemcpyHostToDevice);
    for (size_t i = 0; i < n; ++i) {
        const f16 v = (f16)(float)gauss();
        memcpy(&h[i], &v, 2);
    }
    hipMemcpy(d_rand_h, h.data(), n * 2, hipMemcpyHostToDevice);
    hipMemset(d_zero, 0, n * 2);
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "set-up failed\n"); return 1; }

    struct Cell { const char* feed; const char* data; Kern k32, k16; const unsigned short* src; int iters, units, nw; };
    const int IR = 32000, IL = 32000, IA = 32000;                             // ~16 - 25 ms per launch
    const Cell cells[] = {
        {"reg", "zeros      ", k_reg<32, true>,  k_reg<16, true>,  d_zero,    IR, 32, 4},
        {"reg", "bf16 N(0,1)", k_reg<32, true>,  k_reg<16, true>,  d_rand_bf, IR, 32, 4},
        {"reg", "f16  N(0,1)", k_reg<32, false>, k_reg<16, false>, d_rand_h,  IR, 32, 4},
        {"lds", "zeros      ", k_lds<32, true>,  k_lds<16, true>,  d_zero,    IL, 32, 4},
        {"lds", "bf16 N(0,1)", k_lds<32, true>,  k_lds<16, true>,  d_rand_bf, IL, 32, 4},
        {"lds", "f16  N(0,1)", k_lds<32, false>, k_lds<16, false>, d_rand_h,  IL, 32, 4},
        {"attn", "zeros bf16 ", k_attn<32, true>,  k_attn<16, true>,  d_zero,    IA, 16, 8},
        {"attn", "zeros f16  ", k_attn<32, false>, k_attn<16, false>, d_zero,    IA, 16, 8},
        {"attn", "bf16 N(0,1)", k_attn<32, true>,  k_attn<16, true>,  d_rand_bf, IA, 16, 8},
        {"attn", "f16  N(0,1)", k_attn<32, false>, k_attn<16, false>, d_rand_h,  IA, 16, 8},
    };
    printf("MFMA shape against sustained clock: %d CUs, four waves per CU, median of 5 launches per cell\n", ncu);
    printf("cyc = wave cycles per 32768 flop (one 32x32x16 MFMA, two 16x16x32); GHz = wave cycles / wall time\n");
    printf("feed attn: eight waves per CU in two groups one barrier apart, M slot against V slot; cyc = wave cycles per 64-key TILE (V slot + M slot)\n");
    printf("%-5s %-4s %-12s | %9s %7s %6s | %9s %7s %6s | %s\n", "sweep", "feed", "operands", "32x32x16", "cyc", "GHz", "16x16x32", "cyc", "GHz",
           "TFLOP/s ratio 16x16x32 / 32x32x16");
    for (int sweep = 0; sweep < 2; ++sweep)
        for (const Cell& c : cells) {
            Res a = run(c.k32, c.src, out, cyc, ncu, c.iters, c.units, c.nw);
            Res b = run(c.k16, c.src, out, cyc, ncu, c.iters, c.units, c.nw);
            const Res a2 = run(c.k32, c.src, out, cyc, ncu, c.iters, c.units, c.nw);   // the first shape again: drift inside the cell
            if (c.nw == 8) { a.cyc *= c.units; b.cyc *= c.units; }             // per tile
            printf("%-5d %-4s %-12s | %9.1f %7.2f %6.3f | %9.1f %7.2f %6.3f | %.3f   (32x32x16 again: %.1f TFLOP/s, %.3f GHz)\n", sweep, c.feed, c.data,
                   a.tflops, a.cyc, a.ghz, b.tflops, b.cyc, b.ghz, b.tflops / (0.5 * (a.tflops + a2.tflops)), a2.tflops, a2.ghz);
            fflush(stdout);
        }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "run failed\n"); return 1; }
    return 0;
}
