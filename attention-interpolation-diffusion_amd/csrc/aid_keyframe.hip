// Key-frame K / V^T rows between a processor call and up to AID_KF_MAX_ROWS key-frame stores (aid_keyframe_rows, include/aid_hip.h).
//
// A key-frame store of one layer holds ONE frame: k_store [n_steps, k_fs], vt_store [n_steps, vt_fs] — half of the pair slot of
// aid_endpoint.hip.  Every key frame has its own allocation, so the launch takes a small table (store pointers, row) by value in its
// kernel arguments.  For entry i:
//
//   PUT (call -> store)  reads   k[row_i * k_fs .. +k_fs), vt[row_i * vt_fs .. +vt_fs) and the one int32 *step
//                        writes  k_store_i[*step * k_fs .. +k_fs), vt_store_i[*step * vt_fs .. +vt_fs)
//   GET (store -> call)  reads what PUT writes (and *step), writes what PUT reads.
//
// Nothing else is touched; the whole block moves, gap rows and V^T pad columns included, as aid_endpoint_rows moves them.  The slot
// index is read from DEVICE memory by the kernel: a launch captured into a graph addresses whichever slot the index names at replay
// time, with no node update.  An index outside [0, n_steps) moves nothing.
//
// Pure streaming: the element type does not matter, a lane moves 16 bytes per trip (one vector load, one vector store) on a
// grid-stride walk over the nk + nv chunks of its entry's two blocks.  blockIdx.y is the entry, so the table is indexed uniformly
// per workgroup (scalar loads from the kernel arguments).  No LDS, no atomics.
#include "aid_kernels.hpp"

namespace aid {

struct KeyframeTable {
    uint4*  k_store[AID_KF_MAX_ROWS];
    uint4*  vt_store[AID_KF_MAX_ROWS];
    int32_t row[AID_KF_MAX_ROWS];
};

// nk / nv: 16-byte chunks of one k / vt block (= chunk strides of the rows of k / vt and of the steps of a store)
__global__ __launch_bounds__(256) void aid_keyframe_rows_kernel(uint4* __restrict__ k, uint4* __restrict__ vt, KeyframeTable tab,
                                                                const int32_t* __restrict__ step, int n_steps, int64_t nk, int64_t nv,
                                                                int put) {
    const int st = *step;
    if (st < 0 || st >= n_steps) return;                       // memory-safety guard: the host keeps the index in range
    const int e = blockIdx.y;                                  // gridDim.y == n_rows <= AID_KF_MAX_ROWS
    uint4* const ks = tab.k_store[e] + (int64_t)st * nk;
    uint4* const vs = tab.vt_store[e] + (int64_t)st * nv;
    uint4* const kc = k + (int64_t)tab.row[e] * nk;
    uint4* const vc = vt + (int64_t)tab.row[e] * nv;
    const int64_t total = nk + nv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        uint4* const call = i < nk ? kc + i : vc + (i - nk);
        uint4* const slot = i < nk ? ks + i : vs + (i - nk);
        if (put) *slot = *call;
        else     *call = *slot;
    }
}

hipError_t keyframe_rows_launch(const AidKeyframeRows& a, hipStream_t stream) {
    const int64_t es = a.dtype == AID_DTYPE_F32 ? 4 : 2;
    const int64_t nk = a.k_fs * es / 16, nv = a.vt_fs * es / 16;
    KeyframeTable tab;
    for (int i = 0; i < AID_KF_MAX_ROWS; ++i) {
        const AidKeyframeRow& r = a.rows[i < a.n_rows ? i : 0];       // (unused entries repeat entry 0; no block reads them)
        tab.k_store[i] = static_cast<uint4*>(r.k_store);
        tab.vt_store[i] = static_cast<uint4*>(r.vt_store);
        tab.row[i] = r.row;
    }
    const int64_t blocks = (nk + nv + 255) / 256;
    const int bx = (int)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(aid_keyframe_rows_kernel, dim3(bx, a.n_rows), dim3(256), 0, stream, static_cast<uint4*>(a.k),
                       static_cast<uint4*>(a.vt), tab, a.step, a.n_steps, nk, nv, a.direction == AID_KF_PUT ? 1 : 0);
    return hipGetLastError();
}

}  // namespace aid
