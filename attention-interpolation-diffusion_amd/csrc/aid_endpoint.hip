// End-point K / V^T rows between a processor call and the end-point store (aid_endpoint_rows, include/aid_hip.h).
//
// The store keeps, per self-attention layer, the projected keys and transposed values of the two end-point frames for every AID
// step of a run:  k_store [n_steps, 2, k_fs],  vt_store [n_steps, 2, vt_fs]  (entry 0 = begin, 1 = end).  One launch moves the four
// contiguous blocks of ONE step between that slot and rows row_begin / row_end of a call's k / vt tensors:
//
//   PUT (call -> store)  reads   k[row_begin * k_fs .. +k_fs), k[row_end * k_fs .. +k_fs), vt[row_begin * vt_fs .. +vt_fs),
//                                vt[row_end * vt_fs .. +vt_fs)  and the one int32 *step
//                        writes  k_store[(2 * *step + e) * k_fs .. +k_fs), vt_store[(2 * *step + e) * vt_fs .. +vt_fs), e = 0, 1
//   GET (store -> call)  reads what PUT writes (and *step), writes what PUT reads.
//
// Nothing else is touched; the whole block moves, gap rows and V^T pad columns included (as aid_lerp_kv lerps them).  The slot index
// is read from DEVICE memory by the kernel, like the coefficient buffers of the attention kernels: a launch captured into a graph
// addresses whichever slot the index names at replay time, with no node update.  An index outside [0, n_steps) moves nothing.
//
// Pure streaming: the element type does not matter, a lane moves 16 bytes per trip (one vector load, one vector store) on a
// grid-stride walk over the 2 (nk + nv) chunks of the four blocks.  No LDS, no atomics.
#include "aid_kernels.hpp"

namespace aid {

// nk / nv: 16-byte chunks of one k / vt block; kb / ke / vb / ve: chunk offsets of rows row_begin / row_end in k / vt
__global__ __launch_bounds__(256) void aid_endpoint_rows_kernel(uint4* __restrict__ k, uint4* __restrict__ vt,
                                                                uint4* __restrict__ k_store, uint4* __restrict__ vt_store,
                                                                const int32_t* __restrict__ step, int n_steps, int64_t nk, int64_t nv,
                                                                int64_t kb, int64_t ke, int64_t vb, int64_t ve, int put) {
    const int st = *step;
    if (st < 0 || st >= n_steps) return;                       // memory-safety guard: the host keeps the index in range
    uint4* const ks = k_store + (int64_t)st * 2 * nk;          // slot: [begin block ; end block]
    uint4* const vs = vt_store + (int64_t)st * 2 * nv;
    const int64_t total = 2 * (nk + nv);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        uint4* call;
        uint4* slot;
        if (i < 2 * nk) {
            const bool e = i >= nk;
            const int64_t j = e ? i - nk : i;
            call = k + (e ? ke : kb) + j;
            slot = ks + i;
        } else {
            const int64_t iv = i - 2 * nk;
            const bool e = iv >= nv;
            const int64_t j = e ? iv - nv : iv;
            call = vt + (e ? ve : vb) + j;
            slot = vs + iv;
        }
        if (put) *slot = *call;
        else     *call = *slot;
    }
}

hipError_t endpoint_rows_launch(const AidEndpointRows& a, hipStream_t stream) {
    const int64_t es = a.dtype == AID_DTYPE_F32 ? 4 : 2;
    const int64_t nk = a.k_fs * es / 16, nv = a.vt_fs * es / 16;
    const int64_t total = 2 * (nk + nv);
    const int64_t blocks = (total + 255) / 256;
    const int bx = (int)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(aid_endpoint_rows_kernel, dim3(bx), dim3(256), 0, stream, static_cast<uint4*>(a.k), static_cast<uint4*>(a.vt),
                       static_cast<uint4*>(a.k_store), static_cast<uint4*>(a.vt_store), a.step, a.n_steps, nk, nv,
                       (int64_t)a.row_begin * nk, (int64_t)a.row_end * nk, (int64_t)a.row_begin * nv, (int64_t)a.row_end * nv,
                       a.direction == AID_EP_PUT ? 1 : 0);
    return hipGetLastError();
}

}  // namespace aid
