// The INNER mix of a corner-weighted call read straight from key-frame stores (aid_mix_kv_stores, include/aid_hip.h):
//
//   k2[i] = sum_m w[i, m] K_m[*step]     vt2[i] = sum_m w[i, m] V^T_m[*step]     for the first n_mix frames
//
// with K_m / V^T_m block row *step of key frame m's store — aid_keyframe_rows[_q8] GET of the M rows followed by aid_mix_kv on them, in
// one launch and without the M rows in between.  A lane takes ONE 16-byte chunk position of the call tensor, loads that chunk of all
// M stores once and writes every frame's mix from registers (mix_chunk, aid_mix.hpp: the arithmetic of aid_mix_kv, bit for bit):
//
//   reads   block row *step of the M k stores and the M vt stores, the one int32 *step, w[0 .. n_mix * M)
//   writes  k2[f * k_fs .. + k_fs), vt2[f * vt_fs .. + vt_fs) for f < n_mix — whole blocks, gap rows and pad columns included
//
//   native stores  [n_steps, k_fs] / [n_steps, vt_fs] elements: one 16-byte load per store.
//   q8 stores      [n_steps, aid_q8_block_bytes(.)] bytes (aid_keyframe_q8.hip): the lane's 8 (f16 / bf16) or 4 (f32) int8 and its
//                  block's exponent byte; the value is q * 2^e as GET leaves it in the call dtype.  A GET needs no lane exchange, so
//                  there are no lane groups here.  V^T pad columns (column >= vt_cols of a row of vt_ld) enter as +0: "the first
//                  `keep` elements of the chunk are stored", as there.
//
// The store pointers travel by value in the kernel arguments (indexed by the unrolled corner loop: scalar registers).  The slot index
// is read from DEVICE memory once, uniform; an index outside [0, n_steps) writes nothing.  Grid-stride, 16-byte vector stores, no
// LDS, no atomics.  Compiled without fast-math and without contraction (csrc/Makefile), as aid_corners.o is.
#include "aid_common.hpp"
#include "aid_kernels.hpp"
#include "aid_mix.hpp"

namespace aid {

struct KeyframeBlendTable {
    const uint8_t* k_store[AID_MAX_CORNERS];
    const uint8_t* vt_store[AID_MAX_CORNERS];
};

// the fp32 image of a q8 chunk as GET rounds it to T: EPC int8 in `w`, the first `keep` of them stored, scale = 2^e
template <typename T>
__device__ __forceinline__ typename Chunk<T>::F q8_chunk(const uint8_t* __restrict__ sq, const uint8_t* __restrict__ se, int keep) {
    constexpr int EPC = Chunk<T>::E;
    uint32_t w[EPC / 4];
    if constexpr (EPC == 8) {
        const uint2 q = *reinterpret_cast<const uint2*>(sq);
        w[0] = q.x; w[1] = q.y;
    } else {
        w[0] = *reinterpret_cast<const uint32_t*>(sq);
    }
    const float scale = __builtin_bit_cast(float, (uint32_t)*se << 23);
    typename Chunk<T>::F y;
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
        const int q = (int)(int8_t)(w[j >> 2] >> (8 * (j & 3)));
        float v = j < keep ? (float)q * scale : 0.0f;
        if constexpr (__is_same(T, f16)) v = (float)(f16)v;      // GET's rounding to f16 (exact but at the ends of its range)
        y[j] = v;
    }
    return y;
}

// k_sb / vt_sb: BYTES of one block row of a store (the step stride);
// k_fs / vt_fs: elements of a block (q8: = byte offset of its exponent bytes); vt_cpr: chunks per V^T row (q8)
template <typename T, int M, bool Q8>
__global__ __launch_bounds__(256) void aid_mix_kv_stores_kernel(KeyframeBlendTable tab, T* __restrict__ k2, T* __restrict__ vt2,
                                                                const float* __restrict__ w, const int32_t* __restrict__ step,
                                                                int n_steps, int n_mix, int64_t k_sb, int64_t vt_sb, int64_t k_fs,
                                                                int64_t vt_fs, int vt_cpr, int vt_cols) {
    typedef Chunk<T> C;
    constexpr int E = C::E;
    constexpr int LPB = 32 / E;                                // q8: chunks per block of 32
    const int st = *step;
    if (st < 0 || st >= n_steps) return;                       // memory-safety guard: the host keeps the index in range
    const bool padded = Q8 && vt_cols < vt_cpr * E;
    mix_walk<T, M>([&](int m, bool isk, int64_t j) {           // j: element of its block, c = j / E its chunk
        const uint8_t* const s = (isk ? tab.k_store[m] : tab.vt_store[m]) + (int64_t)st * (isk ? k_sb : vt_sb);
        if constexpr (Q8) {
            const int64_t c = j / E;
            int keep = E;                                      // the first `keep` elements of the chunk are stored
            if (padded && !isk) {
                const int col0 = (int)(c <= 0xffffffffll ? (uint32_t)c % (uint32_t)vt_cpr : c % vt_cpr) * E;
                keep = vt_cols - col0 < 0 ? 0 : vt_cols - col0 > E ? E : vt_cols - col0;
            }
            return q8_chunk<T>(s + j, s + (isk ? k_fs : vt_fs) + c / LPB, keep);
        } else {
            return C::up(*reinterpret_cast<const typename C::V*>(s + j * (int64_t)sizeof(T)));
        }
    }, k2, vt2, w, n_mix, k_fs, vt_fs);
}

template <typename T, int M, bool Q8>
static void blend_launch_m(const KeyframeBlendTable& tab, const MixStoresArgs& a, hipStream_t stream) {
    constexpr int E = Chunk<T>::E;
    const int64_t nk = a.k_fs / E, nv = a.vt_fs / E;
    const int64_t blocks = (nk + nv + 255) / 256;
    const int bx = (int)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);          // the cap of aid_mix_kv's launch
    const int64_t k_sb = Q8 ? (int64_t)aid_q8_block_bytes(a.k_fs) : a.k_fs * (int64_t)sizeof(T);
    const int64_t vt_sb = Q8 ? (int64_t)aid_q8_block_bytes(a.vt_fs) : a.vt_fs * (int64_t)sizeof(T);
    hipLaunchKernelGGL((aid_mix_kv_stores_kernel<T, M, Q8>), dim3(bx), dim3(256), 0, stream, tab, (T*)a.k2, (T*)a.vt2, a.weights, a.step,
                       a.n_steps, a.n_mix, k_sb, vt_sb, a.k_fs, a.vt_fs, Q8 ? a.vt_ld / E : 1, a.vt_cols);
}

template <typename T, bool Q8>
static void blend_launch_t(const KeyframeBlendTable& tab, const MixStoresArgs& a, hipStream_t stream) {
    switch (a.n_corners) {
        case 1: blend_launch_m<T, 1, Q8>(tab, a, stream); break;
        case 2: blend_launch_m<T, 2, Q8>(tab, a, stream); break;
        case 3: blend_launch_m<T, 3, Q8>(tab, a, stream); break;
        case 4: blend_launch_m<T, 4, Q8>(tab, a, stream); break;
        case 5: blend_launch_m<T, 5, Q8>(tab, a, stream); break;
        case 6: blend_launch_m<T, 6, Q8>(tab, a, stream); break;
        case 7: blend_launch_m<T, 7, Q8>(tab, a, stream); break;
        default: blend_launch_m<T, 8, Q8>(tab, a, stream); break;
    }
}

// arguments checked by the caller (1 <= n_corners <= AID_MAX_CORNERS, n_mix >= 0); n_mix == 0 launches nothing
hipError_t mix_kv_stores_launch(const MixStoresArgs& a, hipStream_t stream) {
    if (a.n_mix < 1) return hipSuccess;
    KeyframeBlendTable tab;
    for (int m = 0; m < AID_MAX_CORNERS; ++m) {
        const AidKeyframeRow& r = a.rows[m < a.n_corners ? m : 0];        // (unused entries repeat entry 0; nothing reads them)
        tab.k_store[m] = static_cast<const uint8_t*>(r.k_store);
        tab.vt_store[m] = static_cast<const uint8_t*>(r.vt_store);
    }
    if (a.q8) {
        if (a.dtype == AID_DTYPE_F16)       blend_launch_t<f16, true>(tab, a, stream);
        else if (a.dtype == AID_DTYPE_BF16) blend_launch_t<bf16, true>(tab, a, stream);
        else                                blend_launch_t<float, true>(tab, a, stream);
    } else {
        if (a.dtype == AID_DTYPE_F16)       blend_launch_t<f16, false>(tab, a, stream);
        else if (a.dtype == AID_DTYPE_BF16) blend_launch_t<bf16, false>(tab, a, stream);
        else                                blend_launch_t<float, false>(tab, a, stream);
    }
    return hipGetLastError();
}

}  // namespace aid
