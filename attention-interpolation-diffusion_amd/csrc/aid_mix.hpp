// The corner mix, shared by aid_mix_kv_kernel (aid_corners.hip: the corners are rows of the call's k / vt) and
// aid_mix_kv_stores_kernel (aid_keyframe_blend.hip: the corners are block rows of key-frame stores).  The kernels differ only in how
// corner m's chunk is loaded; the walk, the arithmetic, its order and the stores are this one piece of code.  Both objects are
// compiled without fast-math and without floating-point contraction (csrc/Makefile): the multiplies and adds below are the
// arithmetic as written — a compiler-chosen fused multiply-add would round  p + err  of the f32 path as  fma(w, x, err)  in one kernel
// and not in the other, and the two must agree bit for bit.
#pragma once
#include "aid_common.hpp"

namespace aid {

template <typename T> struct Chunk {                     // one 16-byte chunk of T and its fp32 image
    typedef typename Vec<T>::v8 V;
    typedef f32x8 F;
    static constexpr int E = 8;
    static __device__ __forceinline__ F up(const V& x) { return up8<T>(x); }
    static __device__ __forceinline__ V down(const F& x) { return cvt8<T>(x); }
};
template <> struct Chunk<float> {
    typedef f32x4 V;
    typedef f32x4 F;
    static constexpr int E = 4;
    static __device__ __forceinline__ F up(const V& x) { return x; }
    static __device__ __forceinline__ V down(const F& x) { return x; }
};

// k2[f] = sum_m w[f, m] * corner m's k block, vt2[f] likewise, for f < n_mix: a grid-stride walk over the 16-byte chunk positions of
// the k_fs + vt_fs block.  load(m, isk, j) gives the fp32 image of the chunk at element j of corner m's k (isk) or vt block; a lane loads
// it for all M corners once and writes every frame's mix from registers.  Products and sum in fp32, in corner order, one rounding to
// T; a weight of exactly 0 is skipped (uniform branch); f32 storage carries the rounding errors along (two-sum / fma residuals) and
// adds them before the store.
template <typename T, int M, typename Load>
__device__ __forceinline__ void mix_walk(const Load& load, T* __restrict__ k2, T* __restrict__ vt2, const float* __restrict__ w, int n_mix,
                                         int64_t k_fs, int64_t vt_fs) {
    typedef Chunk<T> C;
    typedef typename C::V V;
    typedef typename C::F F;
    constexpr int E = C::E;
    constexpr bool exact = sizeof(T) == 4;                  // f32 storage: carry the rounding errors (see above)
    const int64_t nk = k_fs / E, nv = vt_fs / E;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nk + nv; i += (int64_t)gridDim.x * blockDim.x) {
        const bool isk = i < nk;
        const int64_t j = (isk ? i : i - nk) * E;
        T* const dst = isk ? k2 : vt2;
        const int64_t fs = isk ? k_fs : vt_fs;
        F x[M];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = load(m, isk, j);
        for (int f = 0; f < n_mix; ++f) {
            F y, err;
#pragma unroll
            for (int e = 0; e < E; ++e) { y[e] = 0.f; err[e] = 0.f; }
            bool first = true;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float wm = w[(int64_t)f * M + m];     // uniform
                if (wm == 0.f) continue;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if (!exact) {
                        y[e] = first ? wm * x[m][e] : fmaf(wm, x[m][e], y[e]);
                    } else {
                        const float p = wm * x[m][e];
                        const float pe = fmaf(wm, x[m][e], -p);             // p + pe == wm * x exactly
                        if (first) { y[e] = p; err[e] = pe; }
                        else {
                            const float s = y[e] + p;
                            const float bb = s - y[e];
                            err[e] += ((y[e] - (s - bb)) + (p - bb)) + pe;  // two-sum: s + (...) == y + p exactly
                            y[e] = s;
                        }
                    }
                }
                first = false;
            }
            if (exact) {
#pragma unroll
                for (int e = 0; e < E; ++e) y[e] += err[e];
            }
            *reinterpret_cast<V*>(dst + (int64_t)f * fs + j) = C::down(y);
        }
    }
}

}  // namespace aid
