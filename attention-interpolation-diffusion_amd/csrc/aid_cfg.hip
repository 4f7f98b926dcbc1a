// Classifier-free guidance with the guidance rescale of arXiv 2305.08891 §3.4 in ONE launch (aid_cfg_rescale, include/aid_hip.h).
// Per sample i, over the e elements of the sample, all arithmetic in fp32:
//   c   = u + gs (t - u)                        t = text[i], u = uncond[i]
//   s_t = std(t), s_c = std(c)                  unbiased, as torch.std
//   out = c (phi s_t / s_c + (1 - phi))         one rounding to T
//
// One workgroup per sample (a run has 3 - 16 samples of 32 - 130 KB: the launch is latency-bound however it is built, and a
// multi-workgroup reduction would add a second launch or an inter-workgroup hand-off to save nothing).  The workgroup walks its
// sample three times — sums, centred squares, output — re-reading t and u from L2 (a sample's two inputs are at most 512 KB):
//   pass 1   sum t, sum c                        -> the two means
//   pass 2   sum (t - mean_t)^2, sum (c - mean_c)^2     (two-pass variance: no cancellation of sum x^2 - (sum x)^2 / e)
//   pass 3   out = c * factor
// The sums take c from one fmaf: its error is 2^-24 of the LARGER of |u| and gs |t - u|, which is nothing to a sum.  The output does
// not: where the guided value nearly cancels (|c| << |u|: u = 3, t = 2.6, gs = 7.5) that error is many units in the last place of c
// itself, so pass 3 forms c with error-free transformations (two-sum of t - u and of the final sum, the product's error from an
// fma) and every element of out is one rounding away from the exact c * factor whatever cancels.  A lane owns the same elements in every
// pass; it reads an element of t and u before it writes that element of out, and the first store of the workgroup comes after the
// barrier that closes the second reduction: out may be t or u itself (same base and stride).  The n - 1 of the unbiased variances
// cancels in s_t / s_c.
// Loads and stores are 16 bytes where the three sample bases are 16-byte aligned (checked per sample: with a stride that is no
// multiple of 16 bytes some samples are, some are not); e % V elements, or the whole sample, go through the scalar loop.
// LDS: the reduction scratch only (two floats per wave).  No atomics, no scratch memory.
#include "aid_common.hpp"
#include "aid_kernels.hpp"

namespace aid {

constexpr int CFG_THREADS = 1024;

template <typename T> struct CfgVec { static constexpr int V = 8; typedef typename Vec<T>::v8 type; };
template <> struct CfgVec<float> { static constexpr int V = 4; typedef f32x4 type; };

template <typename T, int V>
__device__ __forceinline__ void cfg_load(const T* p, float (&v)[V]) {
    const typename CfgVec<T>::type x = *reinterpret_cast<const typename CfgVec<T>::type*>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (float)x[j];
}

template <typename T, int V>
__device__ __forceinline__ void cfg_store(T* p, const float (&v)[V]) {
    typename CfgVec<T>::type x;
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = (T)v[j];                                   // RNE, one rounding
    *reinterpret_cast<typename CfgVec<T>::type*>(p) = x;
}

// u + gs (t - u), correctly rounded to fp32 but for the last addition: a - b = d + dl and p + b = s + sl exactly (Knuth's two-sum),
// gs d = p + pl exactly (fma).  The translation unit is compiled with fast-math; reassociation would cancel the error terms away.
__device__ __forceinline__ float cfg_guided(float gs, float a, float b) {
#pragma clang fp reassociate(off) contract(off)
    const float d = a - b;
    const float bv = d - a;
    const float dl = (a - (d - bv)) + (-b - bv);
    const float p = gs * d;
    const float pl = fmaf(gs, d, -p);
    const float s = p + b;
    const float sv = s - p;
    const float sl = (p - (s - sv)) + (b - sv);
    return s + fmaf(gs, dl, sl + pl);
}

// sums of a and b over the workgroup, returned to every lane; `part` [2][16] is reused by the next call (leading barrier)
__device__ __forceinline__ void cfg_block_sum2(float& a, float& b, float (*part)[CFG_THREADS / 64]) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) {
        part[0][wave] = a;
        part[1][wave] = b;
    }
    __syncthreads();
    a = 0.f;
    b = 0.f;
    for (int w = 0; w < nw; ++w) {          // every lane adds the waves in the same order: one value for the whole workgroup
        a += part[0][w];
        b += part[1][w];
    }
}

// blockDim.x = 64 .. 1024 (a multiple of 64), gridDim.x = n
template <typename T>
__global__ __launch_bounds__(CFG_THREADS) void aid_cfg_rescale_kernel(const T* text, const T* uncond, T* out, int64_t e,
                                                                     int64_t text_stride, int64_t uncond_stride,
                                                                     int64_t out_stride, float gs, float phi) {
    constexpr int V = CfgVec<T>::V;
    __shared__ float part[2][CFG_THREADS / 64];
    const T* t = text + (int64_t)blockIdx.x * text_stride;
    const T* u = uncond + (int64_t)blockIdx.x * uncond_stride;
    T* o = out + (int64_t)blockIdx.x * out_stride;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(o)) & 15) == 0;
    const int64_t nv = vec ? e / V : 0;            // 16-byte chunks; elements [nv V, e) are the scalar loop's

    // pass 1: means
    float st = 0.f, sc = 0.f;
    for (int64_t i = tid; i < nv; i += nthr) {
        float a[V], b[V];
        cfg_load<T, V>(t + i * V, a);
        cfg_load<T, V>(u + i * V, b);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            st += a[j];
            sc += fmaf(gs, a[j] - b[j], b[j]);
        }
    }
    for (int64_t i = nv * V + tid; i < e; i += nthr) {
        const float a = (float)t[i], b = (float)u[i];
        st += a;
        sc += fmaf(gs, a - b, b);
    }
    cfg_block_sum2(st, sc, part);
    const float mt = st / (float)e, mc = sc / (float)e;

    // pass 2: centred squares
    float qt = 0.f, qc = 0.f;
    for (int64_t i = tid; i < nv; i += nthr) {
        float a[V], b[V];
        cfg_load<T, V>(t + i * V, a);
        cfg_load<T, V>(u + i * V, b);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float dt = a[j] - mt, dc = fmaf(gs, a[j] - b[j], b[j]) - mc;
            qt = fmaf(dt, dt, qt);
            qc = fmaf(dc, dc, qc);
        }
    }
    for (int64_t i = nv * V + tid; i < e; i += nthr) {
        const float a = (float)t[i], b = (float)u[i];
        const float dt = a - mt, dc = fmaf(gs, a - b, b) - mc;
        qt = fmaf(dt, dt, qt);
        qc = fmaf(dc, dc, qc);
    }
    cfg_block_sum2(qt, qc, part);                  // (its second barrier is the one every store below stands behind)
    const float factor = fmaf(phi, sqrtf(qt / qc), 1.f - phi);      // s_t / s_c: the e - 1 of both variances cancels

    // pass 3: the guided, rescaled noise
    for (int64_t i = tid; i < nv; i += nthr) {
        float a[V], b[V];
        cfg_load<T, V>(t + i * V, a);
        cfg_load<T, V>(u + i * V, b);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = cfg_guided(gs, a[j], b[j]) * factor;
        cfg_store<T, V>(o + i * V, a);
    }
    for (int64_t i = nv * V + tid; i < e; i += nthr) {
        const float a = (float)t[i], b = (float)u[i];
        o[i] = (T)(cfg_guided(gs, a, b) * factor);
    }
}

template <typename T>
static void cfg_run(const void* text, const void* uncond, void* out, int n, int64_t e, int64_t ts, int64_t us, int64_t os, float gs,
                    float phi, hipStream_t stream) {
    const int64_t nch = (e + CfgVec<T>::V - 1) / CfgVec<T>::V;
    const int threads = nch >= CFG_THREADS ? CFG_THREADS : (int)((nch + 63) / 64 * 64);
    hipLaunchKernelGGL((aid_cfg_rescale_kernel<T>), dim3(n), dim3(threads), 0, stream, (const T*)text, (const T*)uncond, (T*)out, e, ts,
                       us, os, gs, phi);
}

hipError_t cfg_rescale_launch(const void* text, const void* uncond, void* out, int n, int64_t e, int64_t text_stride,
                              int64_t uncond_stride, int64_t out_stride, float gs, float phi, int dtype, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (dtype == AID_DTYPE_F16)       cfg_run<f16>(text, uncond, out, n, e, text_stride, uncond_stride, out_stride, gs, phi, stream);
    else if (dtype == AID_DTYPE_BF16) cfg_run<bf16>(text, uncond, out, n, e, text_stride, uncond_stride, out_stride, gs, phi, stream);
    else                              cfg_run<float>(text, uncond, out, n, e, text_stride, uncond_stride, out_stride, gs, phi, stream);
    return hipGetLastError();
}

}  // namespace aid
