// Key-frame K / V^T rows between a processor call and up to AID_KF_MAX_ROWS 8-bit block stores (aid_keyframe_rows_q8,
// include/aid_hip.h) — aid_keyframe.hip with a quantiser in the lane.
//
// A q8 store of one layer holds ONE frame: k_store [n_steps, aid_q8_block_bytes(k_fs)], vt_store [n_steps, aid_q8_block_bytes(vt_fs)]
// BYTES.  One block row of n elements is n int8, then one exponent byte per 32 consecutive elements, then bytes up to the 16-byte
// boundary that this file neither reads nor writes.  Per block of 32: a = max |x| over the STORED elements (exact: the comparison
// runs on the fp32 bit patterns), e the smallest integer with 127 * 2^e >= a clamped to [-126, 120], exponent byte e + 127,
// q = clamp(rne(x * 2^-e), -127, 127), and the value that comes back is q * 2^e — exact in every storage dtype.  V^T pad columns
// (column >= vt_cols of a row of vt_ld) are not stored: int8 0, no part in the maximum, +0 after GET.  They may hold NaN; they are
// masked on the raw bits before anything is converted.
//
//   PUT (call -> store)  reads   k[row_i * k_fs .. +k_fs), vt[row_i * vt_fs .. +vt_fs) and the one int32 *step
//                        writes  bytes [0, n + ceil(n / 32)) of block row *step of k_store_i (n = k_fs) and vt_store_i (n = vt_fs)
//   GET (store -> call)  reads what PUT writes (and *step), writes what PUT reads (pad columns: +0).
//
// The walk is a grid-stride walk over 16-byte chunks of the CALL tensor: a lane holds 8 (f16 / bf16) or 4 (f32) elements, the 4 or 8
// lanes of a block sit side by side in one wave and agree on the maximum by lane exchange (two or three __shfl_xor steps).  The chunk
// counts of both blocks are rounded up to whole lane groups, so a group is always in one block; a lane past the end of a short last
// block contributes zeros and moves nothing.  A 16-byte chunk never straddles a V^T row (vt_ld % 8 == 0), and the pad columns are
// the last of their row, so "the first `keep` elements of the chunk are stored" is the whole pad rule.  blockIdx.y is the entry; the
// slot index is read from DEVICE memory, an index outside [0, n_steps) moves nothing.  No LDS, no atomics.
#include "aid_common.hpp"
#include "aid_kernels.hpp"

namespace aid {

struct KeyframeQ8Table {
    uint8_t* k_store[AID_KF_MAX_ROWS];
    uint8_t* vt_store[AID_KF_MAX_ROWS];
    int32_t  row[AID_KF_MAX_ROWS];
};

__device__ __forceinline__ float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// the chunk's elements as fp32 BIT PATTERNS, elements >= keep as +0 (masked before any conversion: a pad may hold NaN)
template <typename T, int EPC>
__device__ __forceinline__ void q8_up(const uint4& raw, int keep, uint32_t (&xb)[EPC]) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xb[j] = j < keep ? w[j] : 0u;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t h = j < keep ? (j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu) : 0u;
            if constexpr (sizeof(T) == 2 && __is_same(T, bf16)) xb[j] = h << 16;
            else xb[j] = f32_bits((float)__builtin_bit_cast(f16, (uint16_t)h));
        }
    }
}

// fp32 values (exactly representable in T) to the chunk
template <typename T, int EPC>
__device__ __forceinline__ uint4 q8_down(const float (&y)[EPC]) {
    uint32_t w[4];
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = f32_bits(y[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t lo, hi;
            if constexpr (__is_same(T, bf16)) {
                lo = f32_bits(y[2 * j]) >> 16;                      // at most 7 significant bits: the low half is zero
                hi = f32_bits(y[2 * j + 1]) >> 16;
            } else {
                lo = __builtin_bit_cast(uint16_t, (f16)y[2 * j]);
                hi = __builtin_bit_cast(uint16_t, (f16)y[2 * j + 1]);
            }
            w[j] = lo | hi << 16;
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// nk / nv: 16-byte chunks of one k / vt block of the call; k_sb / vt_sb: bytes of one block row of a store (the step stride);
// k_fs / vt_fs: elements of a block (= byte offset of its exponent bytes); vt_cpr: chunks per V^T row
template <typename T>
__global__ __launch_bounds__(256) void aid_keyframe_rows_q8_kernel(uint4* __restrict__ k, uint4* __restrict__ vt, KeyframeQ8Table tab,
                                                                   const int32_t* __restrict__ step, int n_steps, int64_t nk, int64_t nv,
                                                                   int64_t k_sb, int64_t vt_sb, int64_t k_fs, int64_t vt_fs, int vt_cpr,
                                                                   int vt_cols, int put) {
    constexpr int EPC = 16 / sizeof(T);                        // elements per chunk = int8 bytes per lane
    constexpr int LPB = 32 / EPC;                              // lanes per block of 32
    const int st = *step;
    if (st < 0 || st >= n_steps) return;                       // memory-safety guard: the host keeps the index in range
    const int e = blockIdx.y;                                  // gridDim.y == n_rows <= AID_KF_MAX_ROWS
    uint8_t* const ks = tab.k_store[e] + (int64_t)st * k_sb;
    uint8_t* const vs = tab.vt_store[e] + (int64_t)st * vt_sb;
    uint4* const kc = k + (int64_t)tab.row[e] * nk;
    uint4* const vc = vt + (int64_t)tab.row[e] * nv;
    const int64_t nkp = (nk + LPB - 1) / LPB * LPB;            // whole lane groups: a group never holds chunks of both blocks
    const int64_t total = nkp + (nv + LPB - 1) / LPB * LPB;
    const bool padded = vt_cols < vt_cpr * EPC;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const bool isk = i < nkp;
        const int64_t c = isk ? i : i - nkp;                   // chunk of its block
        const bool in = c < (isk ? nk : nv);                   // (false: a lane past the end of a short last block)
        uint4* const call = (isk ? kc : vc) + c;
        uint8_t* const sq = (isk ? ks : vs) + c * EPC;         // this lane's int8
        uint8_t* const se = (isk ? ks + k_fs : vs + vt_fs) + c / LPB;   // its block's exponent byte
        int keep = in ? EPC : 0;                               // the first `keep` elements of the chunk are stored
        if (padded && !isk && in) {
            const int col0 = (int)(c <= 0xffffffffll ? (uint32_t)c % (uint32_t)vt_cpr : c % vt_cpr) * EPC;
            keep = vt_cols - col0 < 0 ? 0 : vt_cols - col0 > EPC ? EPC : vt_cols - col0;
        }
        if (put) {
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (in) raw = *call;
            uint32_t xb[EPC];
            q8_up<T, EPC>(raw, keep, xb);
            uint32_t a = 0;                                    // max |x| on the bit patterns: exact, and no float compare sees a NaN
#pragma unroll
            for (int j = 0; j < EPC; ++j) a = max(a, xb[j] & 0x7fffffffu);
#pragma unroll
            for (int o = 1; o < LPB; o <<= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
            // 127 * 2^e0 with e0 = exponent(a) - 6 has the mantissa bits 0x7e0000: one exact compare decides between e0 and e0 + 1
            int eb = (int)(a >> 23) - 6 + ((a & 0x7fffffu) > 0x7e0000u ? 1 : 0);      // e + 127
            eb = eb < 1 ? 1 : eb > 247 ? 247 : eb;
            const float inv = bits_f32((uint32_t)(254 - eb) << 23);                  // 2^-e
            uint32_t w[EPC / 4];
#pragma unroll
            for (int j = 0; j < EPC / 4; ++j) w[j] = 0;
#pragma unroll
            for (int j = 0; j < EPC; ++j) {
                const float r = __builtin_amdgcn_fmed3f(__builtin_rintf(bits_f32(xb[j]) * inv), -127.0f, 127.0f);
                w[j >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (j & 3));
            }
            if (in) {
                if constexpr (EPC == 8) *reinterpret_cast<uint2*>(sq) = make_uint2(w[0], w[1]);
                else                    *reinterpret_cast<uint32_t*>(sq) = w[0];
                if (c % LPB == 0) *se = (uint8_t)eb;
            }
        } else if (in) {
            uint32_t w[EPC / 4];
            if constexpr (EPC == 8) {
                const uint2 q = *reinterpret_cast<const uint2*>(sq);
                w[0] = q.x; w[1] = q.y;
            } else {
                w[0] = *reinterpret_cast<const uint32_t*>(sq);
            }
            const float scale = bits_f32((uint32_t)*se << 23);                       // 2^e
            float y[EPC];
#pragma unroll
            for (int j = 0; j < EPC; ++j) {
                const int q = (int)(int8_t)(w[j >> 2] >> (8 * (j & 3)));
                y[j] = j < keep ? (float)q * scale : 0.0f;
            }
            *call = q8_down<T, EPC>(y);
        }
    }
}

template <typename T>
static hipError_t keyframe_rows_q8_launch_t(const AidKeyframeRowsQ8& a, hipStream_t stream) {
    constexpr int EPC = 16 / sizeof(T), LPB = 32 / EPC;
    const int64_t nk = a.k_fs / EPC, nv = a.vt_fs / EPC;
    KeyframeQ8Table tab;
    for (int i = 0; i < AID_KF_MAX_ROWS; ++i) {
        const AidKeyframeRow& r = a.rows[i < a.n_rows ? i : 0];       // (unused entries repeat entry 0; no block reads them)
        tab.k_store[i] = static_cast<uint8_t*>(r.k_store);
        tab.vt_store[i] = static_cast<uint8_t*>(r.vt_store);
        tab.row[i] = r.row;
    }
    const int64_t total = (nk + LPB - 1) / LPB * LPB + (nv + LPB - 1) / LPB * LPB;
    const int64_t blocks = (total + 255) / 256;
    const int bx = (int)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(aid_keyframe_rows_q8_kernel<T>, dim3(bx, a.n_rows), dim3(256), 0, stream, static_cast<uint4*>(a.k),
                       static_cast<uint4*>(a.vt), tab, a.step, a.n_steps, nk, nv, (int64_t)aid_q8_block_bytes(a.k_fs),
                       (int64_t)aid_q8_block_bytes(a.vt_fs), a.k_fs, a.vt_fs, a.vt_ld / EPC, a.vt_cols, a.direction == AID_KF_PUT ? 1 : 0);
    return hipGetLastError();
}

hipError_t keyframe_rows_q8_launch(const AidKeyframeRowsQ8& a, hipStream_t stream) {
    if (a.dtype == AID_DTYPE_F32) return keyframe_rows_q8_launch_t<float>(a, stream);
    if (a.dtype == AID_DTYPE_BF16) return keyframe_rows_q8_launch_t<bf16>(a, stream);
    return keyframe_rows_q8_launch_t<f16>(a, stream);
}

}  // namespace aid
