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

struct Res { double tflops, ghz, cyc; };
typedef void (*Kern)(const unsigned short*, float*, long long*, int);

// `units` = 32768-flop units (one 32x32x16 MFMA's worth) per trip and wave
Res run(Kern kern, const unsigned short* data, float* out, long long* cyc, int ncu, int iters, int units) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    std::vector<float> ms;
    for (int it = 0; it < 7; ++it) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(ncu), dim3(256), 0, 0, data, out, cyc, iters);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float t; hipEventElapsedTime(&t, e0, e1);
        if (it >= 2) ms.push_back(t);                                         // two launches let the clock settle
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    std::vector<long long> hc(ncu * 4);
    hipMemcpy(hc.data(), cyc, hc.size() * sizeof(long long), hipMemcpyDeviceToHost);
    double cs = 0; for (auto c : hc) cs += (double)c;
    cs /= hc.size();
    hipEventDestroy(e0); hipEventDestroy(e1);
    const double u = (double)iters * units;
    Res r;
    r.tflops = u * 4 * ncu * 32768.0 / (med * 1e-3) / 1e12;
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
    hipMalloc(&out, (size_t)ncu * 256 * 4); hipMalloc(&cyc, (size_t)ncu * 4 * sizeof(long long));
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

    struct Cell { const char* feed; const char* data; Kern k32, k16; const unsigned short* src; int iters, units; };
    const int IR = 32000, IL = 32000;                                         // ~16 - 25 ms per launch
    const Cell cells[] = {
        {"reg", "zeros      ", k_reg<32, true>,  k_reg<16, true>,  d_zero,    IR, 32},
        {"reg", "bf16 N(0,1)", k_reg<32, true>,  k_reg<16, true>,  d_rand_bf, IR, 32},
        {"reg", "f16  N(0,1)", k_reg<32, false>, k_reg<16, false>, d_rand_h,  IR, 32},
        {"lds", "zeros      ", k_lds<32, true>,  k_lds<16, true>,  d_zero,    IL, 32},
        {"lds", "bf16 N(0,1)", k_lds<32, true>,  k_lds<16, true>,  d_rand_bf, IL, 32},
        {"lds", "f16  N(0,1)", k_lds<32, false>, k_lds<16, false>, d_rand_h,  IL, 32},
    };
    printf("MFMA shape against sustained clock: %d CUs, four waves per CU, median of 5 launches per cell\n", ncu);
    printf("cyc = wave cycles per 32768 flop (one 32x32x16 MFMA, two 16x16x32); GHz = wave cycles / wall time\n");
    printf("%-5s %-4s %-12s | %9s %7s %6s | %9s %7s %6s | %s\n", "sweep", "feed", "operands", "32x32x16", "cyc", "GHz", "16x16x32", "cyc", "GHz",
           "TFLOP/s ratio 16x16x32 / 32x32x16");
    for (int sweep = 0; sweep < 2; ++sweep)
        for (const Cell& c : cells) {
            const Res a = run(c.k32, c.src, out, cyc, ncu, c.iters, c.units);
            const Res b = run(c.k16, c.src, out, cyc, ncu, c.iters, c.units);
            const Res a2 = run(c.k32, c.src, out, cyc, ncu, c.iters, c.units);   // the first shape again: drift inside the cell
            printf("%-5d %-4s %-12s | %9.1f %7.2f %6.3f | %9.1f %7.2f %6.3f | %.3f   (32x32x16 again: %.1f TFLOP/s, %.3f GHz)\n", sweep, c.feed, c.data,
                   a.tflops, a.cyc, a.ghz, b.tflops, b.cyc, b.ghz, b.tflops / (0.5 * (a.tflops + a2.tflops)), a2.tflops, a2.ghz);
            fflush(stdout);
        }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "run failed\n"); return 1; }
    return 0;
}
