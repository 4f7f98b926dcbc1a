// Corner-weighted AID (aid_mix_kv, aid_attn_corners_fwd; include/aid_hip.h): the two kernels the composition over aid_attn_fwd needs.
//
//   aid_mix_kv_kernel        k2[i] = sum_m w[i, m] k[rows[m]]  (same for vt -> vt2) for the first n_mix frames — the INNER mix among
//                            M <= AID_MAX_CORNERS corner rows.  A lane takes ONE 16-byte chunk position of the k_fs + vt_fs block,
//                            loads that chunk of all M corner rows once and writes every frame's mix from registers: the launch
//                            reads M blocks and writes n_mix blocks (not M * n_mix reads).  M is a template parameter, so the M
//                            chunks live in registers (no scratch); the weights are uniform per workgroup (scalar loads).
//                            Products and sum in fp32, in corner order, one rounding to the storage type; a weight of exactly 0 is
//                            skipped (uniform branch), so a one-hot row returns the corner's bits — -0, Inf and NaN included.
//                            f32 storage has no wider accumulator to round from: there the rounding errors of the M products and
//                            sums are carried along (two-sum / fma residuals, still fp32 arithmetic) and added before the store, so
//                            the stored value is within one f32 unit of the exact mix as the 16-bit types are within one of theirs.
//   aid_corner_pairs_kernel  the pair table of aid_attn_corners_fwd, one thread per frame:
//                              tab[i]                      0.5 (AID frame) / -1 (rider)            the INNER coefficient vector
//                              tab[(1 + 2p) n + i]         coef_p[i]  = s > 0 ? b / s : 0          rider: -1
//                              tab[(2 + 2p) n + i]         scale_p[i] = s = a + b                  rider:  1
//                            with a = w[i, 2p], b = (2p + 1 < M) ? w[i, 2p + 1] : 0.  A rider's weight row is not read.
//
// The walk and the arithmetic of the mix are mix_walk (aid_mix.hpp), shared with the store form (aid_keyframe_blend.hip).
// Grid-stride, no LDS, no atomics.  This object is compiled without fast-math and without contraction (csrc/Makefile): the order of the sum, the exact 1 of
// b / (0 + b) and the error terms of the f32 path are arithmetic the compiler must not rewrite.
#include "aid_common.hpp"
#include "aid_kernels.hpp"
#include "aid_mix.hpp"

namespace aid {

template <typename T, int M>
__global__ __launch_bounds__(256) void aid_mix_kv_kernel(const T* __restrict__ k, const T* __restrict__ vt, T* __restrict__ k2,
                                                         T* __restrict__ vt2, const float* __restrict__ w, CornerRows rows, int n_mix,
                                                         int64_t k_fs, int64_t vt_fs) {
    typedef Chunk<T> C;
    mix_walk<T, M>([&](int m, bool isk, int64_t j) {
        return C::up(*reinterpret_cast<const typename C::V*>((isk ? k : vt) + rows.row[m] * (isk ? k_fs : vt_fs) + j));
    }, k2, vt2, w, n_mix, k_fs, vt_fs);
}

__global__ __launch_bounds__(64) void aid_corner_pairs_kernel(const float* __restrict__ w, float* __restrict__ tab, int n_frames,
                                                              int n_mix, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames) return;
    const bool rider = i >= n_mix;
    tab[i] = rider ? -1.f : 0.5f;
    const int P = (M + 1) / 2;
    for (int p = 0; p < P; ++p) {
        float coef = -1.f, scale = 1.f;
        if (!rider) {
            const float a = w[(int64_t)i * M + 2 * p];
            const float b = 2 * p + 1 < M ? w[(int64_t)i * M + 2 * p + 1] : 0.f;
            const float s = a + b;
            coef = s > 0.f ? (a == 0.f ? 1.f : b / s) : 0.f;      // a == 0: exactly 1, whatever the divider does
            scale = s;
        }
        tab[(int64_t)(1 + 2 * p) * n_frames + i] = coef;
        tab[(int64_t)(2 + 2 * p) * n_frames + i] = scale;
    }
}

template <typename T, int M>
static void mix_launch_m(const void* k, const void* vt, void* k2, void* vt2, const float* w, const CornerRows& rows, int n_mix,
                         int64_t k_fs, int64_t vt_fs, hipStream_t stream) {
    const int64_t chunks = (k_fs + vt_fs) / Chunk<T>::E;
    const int64_t blocks = (chunks + 255) / 256;
    const int bx = (int)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL((aid_mix_kv_kernel<T, M>), dim3(bx), dim3(256), 0, stream, (const T*)k, (const T*)vt, (T*)k2, (T*)vt2, w, rows,
                       n_mix, k_fs, vt_fs);
}

template <typename T>
static void mix_launch_t(int m, const void* k, const void* vt, void* k2, void* vt2, const float* w, const CornerRows& rows, int n_mix,
                         int64_t k_fs, int64_t vt_fs, hipStream_t stream) {
    switch (m) {
        case 1: mix_launch_m<T, 1>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 2: mix_launch_m<T, 2>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 3: mix_launch_m<T, 3>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 4: mix_launch_m<T, 4>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 5: mix_launch_m<T, 5>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 6: mix_launch_m<T, 6>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        case 7: mix_launch_m<T, 7>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
        default: mix_launch_m<T, 8>(k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream); break;
    }
}

// arguments checked by the caller (1 <= n_corners <= AID_MAX_CORNERS, n_mix >= 0); n_mix == 0 launches nothing
hipError_t mix_kv_launch(const void* k, const void* vt, void* k2, void* vt2, const float* w, const CornerRows& rows, int n_corners,
                         int n_mix, int64_t k_fs, int64_t vt_fs, int dtype, hipStream_t stream) {
    if (n_mix < 1) return hipSuccess;
    if (dtype == AID_DTYPE_F16)       mix_launch_t<f16>(n_corners, k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream);
    else if (dtype == AID_DTYPE_BF16) mix_launch_t<bf16>(n_corners, k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream);
    else                              mix_launch_t<float>(n_corners, k, vt, k2, vt2, w, rows, n_mix, k_fs, vt_fs, stream);
    return hipGetLastError();
}

hipError_t corner_pairs_launch(const float* w, float* tab, int n_frames, int n_mix, int n_corners, hipStream_t stream) {
    hipLaunchKernelGGL(aid_corner_pairs_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, stream, w, tab, n_frames, n_mix, n_corners);
    return hipGetLastError();
}

}  // namespace aid
