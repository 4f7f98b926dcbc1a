// Row gain of a DoRA adapter (aid_dora_gain, include/aid_hip.h):
//   gain[n] = magnitude[n] / || W[n, :] + (B_pack A_pack)[n, :] ||_2
// PEFT's DoRA layers re-materialise B A and the norm on every forward; the gain depends on weights only, so it is computed once per
// adapter pack and handed to the projection GEMMs (AidGemmProblem.lr_row_scale), which multiply their fp32 accumulators by it.
//
// A workgroup takes DORA_ROWS weight rows.  Their B_pack rows sit in LDS as fp32, [rank][DORA_ROWS], so one 16-byte LDS read gives
// the coefficient of every row for one rank index.  The lanes stride over n_in in 16-byte chunks: a lane holds its chunk of the
// DORA_ROWS rows  t = W + sum_j B[n, j] A[j, chunk]  in registers (fp32 FMAs; A_pack is read once per workgroup, coalesced, from L2),
// squares it, and the sums are reduced in the wave and then across the waves through LDS.  W + B A is never written.  No MFMA (the
// product is [DORA_ROWS, rank] x [rank, n_in] per workgroup and is read-bound), no atomics.
#include "aid_common.hpp"
#include "aid_kernels.hpp"

namespace aid {

constexpr int DORA_ROWS = 4;
constexpr int DORA_MAX_RANK = 512;

// one 16-byte load of E elements, widened to fp32
template <typename T, int E>
__device__ __forceinline__ void load16(const T* p, float (&v)[E]) {
    if constexpr (E == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[e];
    } else {
        const f32x8 x = up8<T>(*reinterpret_cast<const typename Vec<T>::v8*>(p));
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = x[e];
    }
}

__device__ __forceinline__ float dora_wave_sum(float v) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
    return sum_halves(v);
}

// blockDim.x = 64 .. 256 (a multiple of 64: as many waves as the row has 16-byte chunks for)
template <typename T, int E>
__global__ __launch_bounds__(256) void aid_dora_gain_kernel(const T* __restrict__ w, const T* __restrict__ a, const T* __restrict__ b,
                                                            const T* __restrict__ mag, float* __restrict__ gain, int n_out, int n_in,
                                                            int ldw, int rank) {
    __shared__ __attribute__((aligned(16))) float Bs[DORA_MAX_RANK * DORA_ROWS];      // [rank][row]
    __shared__ float part[4][DORA_ROWS];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * DORA_ROWS;
    int rows[DORA_ROWS];                                   // rows past the end: a valid row, its result is dropped
#pragma unroll
    for (int r = 0; r < DORA_ROWS; ++r) rows[r] = min(row0 + r, n_out - 1);
    for (int i = tid; i < rank * DORA_ROWS; i += nthr) {
        const int r = i / rank, j = i - r * rank;          // consecutive lanes read consecutive j of one row
        Bs[j * DORA_ROWS + r] = (float)b[(int64_t)min(row0 + r, n_out - 1) * rank + j];
    }
    __syncthreads();
    float ss[DORA_ROWS];
#pragma unroll
    for (int r = 0; r < DORA_ROWS; ++r) ss[r] = 0.f;
    const int nch = n_in / E;
    for (int ch = tid; ch < nch; ch += nthr) {
        float t[DORA_ROWS][E];
#pragma unroll
        for (int r = 0; r < DORA_ROWS; ++r) load16<T, E>(w + (int64_t)rows[r] * ldw + ch * E, t[r]);
        const T* ap = a + ch * E;
#pragma unroll 4
        for (int j = 0; j < rank; ++j) {
            float av[E];
            load16<T, E>(ap + (int64_t)j * n_in, av);
            const f32x4 bj = *reinterpret_cast<const f32x4*>(Bs + j * DORA_ROWS);
#pragma unroll
            for (int r = 0; r < DORA_ROWS; ++r)
#pragma unroll
                for (int e = 0; e < E; ++e) t[r][e] = fmaf(bj[r], av[e], t[r][e]);
        }
#pragma unroll
        for (int r = 0; r < DORA_ROWS; ++r)
#pragma unroll
            for (int e = 0; e < E; ++e) ss[r] = fmaf(t[r][e], t[r][e], ss[r]);
    }
#pragma unroll
    for (int r = 0; r < DORA_ROWS; ++r) {
        const float s = dora_wave_sum(ss[r]);
        if (lane == 0) part[wave][r] = s;
    }
    __syncthreads();
    if (tid < DORA_ROWS && row0 + tid < n_out) {           // one lane per row: sum over the waves, one store
        float s = 0.f;
        for (int v = 0; v < (nthr >> 6); ++v) s += part[v][tid];
        gain[row0 + tid] = (float)mag[row0 + tid] / sqrtf(s);
    }
}

template <typename T, int E>
static void dora_run(const void* w, const void* a, const void* b, const void* mag, float* gain, int n_out, int n_in, int ldw, int rank,
                     hipStream_t stream) {
    const int nch = n_in / E;
    const int threads = nch >= 256 ? 256 : (nch + 63) / 64 * 64;
    hipLaunchKernelGGL((aid_dora_gain_kernel<T, E>), dim3((n_out + DORA_ROWS - 1) / DORA_ROWS), dim3(threads), 0, stream,
                       (const T*)w, (const T*)a, (const T*)b, (const T*)mag, gain, n_out, n_in, ldw, rank);
}

hipError_t dora_gain_launch(const void* w, const void* a_pack, const void* b_pack, const void* magnitude, float* gain, int n_out,
                            int n_in, int ldw, int rank, int dtype, hipStream_t stream) {
    if (n_out <= 0) return hipSuccess;
    if (rank > DORA_MAX_RANK) return hipErrorInvalidValue;
    if (dtype == AID_DTYPE_F16)       dora_run<f16, 8>(w, a_pack, b_pack, magnitude, gain, n_out, n_in, ldw, rank, stream);
    else if (dtype == AID_DTYPE_BF16) dora_run<bf16, 8>(w, a_pack, b_pack, magnitude, gain, n_out, n_in, ldw, rank, stream);
    else                              dora_run<float, 4>(w, a_pack, b_pack, magnitude, gain, n_out, n_in, ldw, rank, stream);
    return hipGetLastError();
}

}  // namespace aid
