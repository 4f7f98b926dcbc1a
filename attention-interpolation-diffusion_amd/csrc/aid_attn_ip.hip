// IP-Adapter image attention over SEVERAL key segments in one launch (aid_ip_attn_fwd): the de-activated IP-Adapter layer with more
// than one adapter, with regional ip_adapter_masks, or with a text attention_mask (diffusers' IPAdapterAttnProcessor2_0):
//     out[i, s, head] = round( float(out[i, s, head]) + sum_g scale_g * (w_g ? w_g[s] : 1) * softmax(Q K_g^T * scale) V_g )
// Image keys are tiny (4, 16 or 257 tokens per image: K and V^T of every segment of a launch total a few hundred KB and stay in L2),
// so the launch is a stream over Q and out.  aid_attn_fwd(accumulate = 1) adds one segment per launch, i.e. G passes over Q and out,
// and has no per-row weight; here a wave walks all G segments while its 32-row Q tile is in registers: Q is read once, out is read
// once and written once.
//   * a wave owns the 32 x d tile of one (frame, head, row block) and is independent of every other wave: no LDS, no barrier;
//     K and V^T fragments come straight from global memory (L2 / L1 hits after the first wave of a head);
//   * swapped products like aid_attn_tx: S^T[key, row] = K Q^T, O^T[channel, row] = V^T P^T on mfma_f32_32x32x16, so a lane holds one
//     query row's scores and the probabilities leave the softmax already in the B-operand layout of the second product;
//   * one 32-key score tile at a time with an online softmax: t_g has no upper limit; every segment has its own softmax, row sum and
//     fp32 output block, which is added into the result block with  scale_g * w_g[row] / rowsum;
//   * the head dim is padded as in aid_attn_kernel (DK to 16 for the contraction of K Q^T, DV to 32 rows of O^T): pad channels of Q,
//     K and V^T are zeros made in registers, never read;
//   * rows >= t_g of K and columns >= t_g of V^T are never read into arithmetic: K rows past t_g are zeros made in registers and
//     their scores are set to -inf; V^T is read in 4-key pieces whose first key is < t_g (so a piece ends at most at round_up(t_g, 4)
//     <= ldvt) and the elements of keys >= t_g are replaced by zeros;
//   * out leaves as 16-byte stores: two v_permlane32_swap per 16 channels bring the halves of a row together (and the same two swaps
//     bring the 16-byte words of the previous `out` into the accumulator layout); one rounding.
// Registers (the build's resource table, tests/test_ip_multi_abi.py): d = 40 / 64 / 80 keep Q live across the segments (three waves
// per SIMD for 40 / 64, two for 80); d = 160 re-reads its Q fragments per score tile from L1 and walks its channel blocks in two
// passes (two waves per SIMD).  No scratch anywhere.
#include <string.h>

#include <type_traits>

#include "aid_common.hpp"
#include "aid_kernels.hpp"

namespace aid {

struct IpSeg {
    const void*  k;                     // [rows, t, heads * d]
    const void*  vt;                    // [rows, heads * d, ldvt]
    const float* rw;                    // [s] or nullptr
    int64_t k_fs, vt_fs;                // 0 when every frame uses row 0
    int32_t t, ldvt;
    float   scale;
    int32_t pad;
};

struct IpParams {
    const void* q;
    void*       out;
    int64_t q_fs, o_fs;
    int32_t n_frames, s, heads, ldq, ldo, nseg;
    int32_t chunks;                     // workgroups per (frame, head): four 32-row tiles each
    float   c2;                         // softmax_scale * log2(e), or 1 when q is pre-scaled
    IpSeg   seg[AID_IP_MAX_SEGMENTS];
};

__device__ __forceinline__ f32x16 ip_zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

template <typename T>
__device__ __forceinline__ uint32_t ip_pack2(float x, float y) {
    typename Vec<T>::v2 v = __builtin_convertvector((f32x2){x, y}, typename Vec<T>::v2);
    return __builtin_bit_cast(uint32_t, v);
}
template <typename T>
__device__ __forceinline__ f32x2 ip_unpack2(uint32_t w) {
    return __builtin_convertvector(__builtin_bit_cast(typename Vec<T>::v2, w), f32x2);
}

// acc + w.lo + w.hi: the row sum is taken over the ROUNDED probabilities, the numbers the second product multiplies
template <typename T>
__device__ __forceinline__ float ip_dot2(uint32_t w, float acc);
template <>
__device__ __forceinline__ float ip_dot2<bf16>(uint32_t w, float acc) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    b2 one;
    one[0] = (__bf16)1.0f; one[1] = (__bf16)1.0f;
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2, w), one, acc, false);
}
template <>
__device__ __forceinline__ float ip_dot2<f16>(uint32_t w, float acc) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 one;
    one[0] = (_Float16)1.0f; one[1] = (_Float16)1.0f;
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w), one, acc, false);
}

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void aid_ip_attn_kernel(const IpParams p) {
    typedef typename Vec<T>::v8 T8;
    typedef typename Vec<T>::v4 T4;
    constexpr int DK = (D + 15) / 16 * 16;              // contraction length of K Q^T (MFMA k = 16)
    constexpr int DV = (D + 31) / 32 * 32;              // rows of O^T (MFMA m = 32)
    constexpr int NQK = DK / 16, NDB = DV / 32;
    constexpr bool QLIVE = D <= 80;                     // Q fragments stay in registers across the segments
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
    const int id = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int head = id % p.heads, r1 = id / p.heads, chunk = r1 % p.chunks, fr = r1 / p.chunks;
    const int tile = 4 * chunk + wave;
    if (32 * tile >= p.s) return;                       // (wave-uniform: every lane of a running wave stays active for the swaps)
    const bool row_ok = 32 * tile + m < p.s;
    const int row = row_ok ? 32 * tile + m : p.s - 1;   // rows past S: any valid row, their results are not stored
    const T* const qrow = reinterpret_cast<const T*>(p.q) + (int64_t)fr * p.q_fs + (int64_t)row * p.ldq + head * D + 8 * h;
    const int ldk = p.heads * D;
    const float c2 = p.c2;

    auto q_frag = [&](int j) -> T8 {                    // Q[row][16 j + 8 h .. + 7]; channels >= D are zeros
        return (D % 16 == 0 || 16 * j + 8 * h < D) ? *reinterpret_cast<const T8*>(qrow + 16 * j) : zero8<T>();
    };
    T8 qf[QLIVE ? NQK : 1];
    if (QLIVE) {
#pragma unroll
        for (int j = 0; j < NQK; ++j) qf[j] = q_frag(j);
    }

    // one pass = every segment and the store for the 32-channel blocks [CT0, CT0 + NCT) of O^T
    auto pass = [&](auto ct0_c, auto nct_c) {
    constexpr int CT0 = decltype(ct0_c)::value, NCT = decltype(nct_c)::value;
    f32x16 res[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) res[ct] = ip_zero16();

#pragma unroll 1
    for (int g = 0; g < p.nseg; ++g) {
        const IpSeg& sg = p.seg[g];
        const int t = sg.t, ldvt = sg.ldvt;
        const T* const kb = reinterpret_cast<const T*>(sg.k) + (int64_t)fr * sg.k_fs + head * D + 8 * h;
        const T* const vb = reinterpret_cast<const T*>(sg.vt) + (int64_t)fr * sg.vt_fs + (int64_t)(head * D + m) * ldvt + 4 * h;
        f32x16 oc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) oc[ct] = ip_zero16();
        float mx = -INFINITY, ls = 0.f;
        const int nkt = (t + 31) >> 5;
#pragma unroll 1
        for (int kt = 0; kt < nkt; ++kt) {
            // ---- S^T[key, row] = K Q^T for keys 32 kt .. + 31: lane (m, h) supplies K[32 kt + m][16 j + 8 h .. + 7] ----
            const int key = 32 * kt + m;
            const T* const krow = kb + (int64_t)(key < t ? key : 0) * ldk;
            f32x16 sc = ip_zero16();
#pragma unroll
            for (int j = 0; j < NQK; ++j) {
                const bool ok = key < t && (D % 16 == 0 || 16 * j + 8 * h < D);
                const T8 kf = ok ? *reinterpret_cast<const T8*>(krow + 16 * j) : zero8<T>();
                sc = mfma32(kf, QLIVE ? qf[j] : q_frag(j), sc);
            }
            // register i of the lane is key 32 kt + 8 (i / 4) + i % 4 + 4 h
            const int lim = t - 32 * kt - 4 * h;
            const bool edge = 32 * kt + 32 > t;                          // the tile that straddles t: keys >= t to -inf
            if (edge) {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (8 * (i >> 2) + (i & 3) >= lim) sc[i] = -INFINITY;
            }
            float tm = sc[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) tm = fmaxf(tm, sc[i]);
            tm = max_halves(tm);                                         // (key 32 kt < t: the row's maximum is a real score)
            const float mn = fmaxf(mx, tm);
            const float alpha = __builtin_amdgcn_exp2f((mx - mn) * c2);   // first tile: exp2(-inf) = 0 on zeros
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) oc[ct] *= alpha;
            ls *= alpha;
            mx = mn;
            const float nm = -mx * c2;
            // ---- O^T[channel, row] += V^T P^T, 16 keys at a time: the lane's eight probabilities of the step are keys
            //      16 u + 4 h .. + 3 and 16 u + 8 + 4 h .. + 3, so the V^T fragment is those two 4-key pieces ----
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k0 = 32 * kt + 16 * u;
                if (k0 < t) {                                            // (uniform) 16-key steps entirely past t are never read
                    uint32_t pk[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float p0 = __builtin_amdgcn_exp2f(fmaf(sc[8 * u + 2 * e], c2, nm));
                        const float p1 = __builtin_amdgcn_exp2f(fmaf(sc[8 * u + 2 * e + 1], c2, nm));
                        pk[e] = ip_pack2<T>(p0, p1);
                        ls = ip_dot2<T>(pk[e], ls);
                    }
                    const T8 pf = __builtin_bit_cast(T8, (u32x4){pk[0], pk[1], pk[2], pk[3]});
                    const int ka = k0 + 4 * h, kb2 = ka + 8;             // first keys of the lane's two pieces
#pragma unroll
                    for (int cb = 0; cb < NCT; ++cb) {
                        const int ct = CT0 + cb;
                        const bool ch_ok = D == DV || 32 * ct + m < D;   // channels >= D: zero rows of O^T, not stored
                        const T* const src = vb + (int64_t)(32 * ct) * ldvt + k0;
                        T4 va, vc;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { va[e] = (T)0.0f; vc[e] = (T)0.0f; }
                        if (ch_ok && ka < t) va = *reinterpret_cast<const T4*>(src);
                        if (ch_ok && kb2 < t) vc = *reinterpret_cast<const T4*>(src + 8);
                        if (edge) {                                      // keys >= t have P = 0; their V must not be NaN / inf
#pragma unroll
                            for (int e = 1; e < 4; ++e) {
                                if (ka + e >= t) va[e] = (T)0.0f;
                                if (kb2 + e >= t) vc[e] = (T)0.0f;
                            }
                        }
                        const T8 vf = __builtin_shufflevector(va, vc, 0, 1, 2, 3, 4, 5, 6, 7);
                        oc[cb] = mfma32(vf, pf, oc[cb]);
                    }
                }
            }
        }
        ls = sum_halves(ls);
        float w = sg.scale / ls;
        if (sg.rw) w *= sg.rw[row];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) res[ct] += oc[ct] * w;
    }

    // ---- out = round(float(out) + res): lane (row m, half h) holds channels 32 ct + 8 (r / 4) + r % 4 + 4 h; the 16-byte word of
    //      `out` it loads and stores holds channels 32 ct + 16 u + 8 h .. + 7 — the same two swaps convert either way ----
    T* const orow = reinterpret_cast<T*>(p.out) + (int64_t)fr * p.o_fs + (int64_t)row * p.ldo + head * D + 8 * h;
#pragma unroll
    for (int cb = 0; cb < NCT; ++cb)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ct = CT0 + cb;
            if (32 * ct + 16 * u >= D) continue;                        // (compile time) a 16-channel group entirely in the pad
            const bool ok = row_ok && (D % 16 == 0 || 32 * ct + 16 * u + 8 * h < D);
            u32x4 pw = (u32x4){0u, 0u, 0u, 0u};
            if (ok) pw = *reinterpret_cast<const u32x4*>(orow + 32 * ct + 16 * u);
            const auto a0 = __builtin_amdgcn_permlane32_swap(pw[0], pw[2], false, false);
            const auto a1 = __builtin_amdgcn_permlane32_swap(pw[1], pw[3], false, false);
            const f32x2 x0 = ip_unpack2<T>(a0[0]), x1 = ip_unpack2<T>(a1[0]), y0 = ip_unpack2<T>(a0[1]), y1 = ip_unpack2<T>(a1[1]);
            const f32x16& r = res[cb];
            const uint32_t nx0 = ip_pack2<T>(x0[0] + r[8 * u], x0[1] + r[8 * u + 1]);
            const uint32_t nx1 = ip_pack2<T>(x1[0] + r[8 * u + 2], x1[1] + r[8 * u + 3]);
            const uint32_t ny0 = ip_pack2<T>(y0[0] + r[8 * u + 4], y0[1] + r[8 * u + 5]);
            const uint32_t ny1 = ip_pack2<T>(y1[0] + r[8 * u + 6], y1[1] + r[8 * u + 7]);
            const auto s0 = __builtin_amdgcn_permlane32_swap(nx0, ny0, false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(nx1, ny1, false, false);
            if (ok) *reinterpret_cast<u32x4*>(orow + 32 * ct + 16 * u) = (u32x4){s0[0], s1[0], s0[1], s1[1]};
        }
    };
    // d = 160: 80 result + 80 segment accumulators do not fit beside the fragments, so the five channel blocks run as two passes
    // (3 + 2) that compute the scores twice — the d = 160 layers are the smallest of a stack (S <= 256)
    if constexpr (D == 160) {
        pass(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
        pass(std::integral_constant<int, 3>{}, std::integral_constant<int, 2>{});
    } else {
        pass(std::integral_constant<int, 0>{}, std::integral_constant<int, NDB>{});
    }
}

template <typename T, int D>
static hipError_t ip_launch(const IpParams& p, hipStream_t stream) {
    const void* fn = reinterpret_cast<const void*>(&aid_ip_attn_kernel<T, D>);
    const int grid = p.heads * p.n_frames * p.chunks;
    void* kargs[] = {const_cast<IpParams*>(&p)};
    return hipLaunchKernel(fn, dim3(grid), dim3(256), kargs, 0, stream);
}

template <typename T>
static hipError_t ip_launch_d(const IpParams& p, int d, hipStream_t stream) {
    switch (d) {
        case 40: return ip_launch<T, 40>(p, stream);
        case 64: return ip_launch<T, 64>(p, stream);
        case 80: return ip_launch<T, 80>(p, stream);
        case 160: return ip_launch<T, 160>(p, stream);
        default: return hipErrorInvalidValue;
    }
}

// Workgroups of four independent waves, one 32-row tile each: S = 4096 x 8 frames x 10 heads is 2560 workgroups, ten per CU.  The
// kernel hides the latency of its global K / V^T fragments behind the OTHER waves of the SIMD: the launch counts on >= 3 waves per
// SIMD for d = 40 / 64 and on 2 for d = 80 / 160 (no LDS, so registers alone decide).
hipError_t ip_attn_launch(const AidIpAttnArgs& a, hipStream_t stream) {
    IpParams p;
    memset(&p, 0, sizeof(p));
    p.q = a.q; p.out = a.out;
    p.q_fs = a.q_fs; p.o_fs = a.o_fs;
    p.n_frames = a.n_frames; p.s = a.s; p.heads = a.heads; p.ldq = a.ldq; p.ldo = a.ldo;
    p.nseg = a.n_segments;
    p.chunks = ((a.s + 31) / 32 + 3) / 4;
    p.c2 = a.q_prescaled ? 1.f : a.softmax_scale * 1.4426950408889634f;
    for (int g = 0; g < a.n_segments; ++g) {
        const AidIpSegment& s = a.segments[g];
        IpSeg& d = p.seg[g];
        d.k = s.k; d.vt = s.vt; d.rw = s.row_weight;
        d.k_fs = s.n_rows == 1 ? 0 : s.k_fs;
        d.vt_fs = s.n_rows == 1 ? 0 : s.vt_fs;
        d.t = s.t; d.ldvt = s.ldvt; d.scale = s.scale;
    }
    return a.dtype == AID_DTYPE_F16 ? ip_launch_d<f16>(p, a.d, stream) : ip_launch_d<bf16>(p, a.d, stream);
}

}  // namespace aid
