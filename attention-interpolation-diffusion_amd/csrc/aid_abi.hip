// extern "C" boundary of libaid_hip.so (see include/aid_hip.h).  Argument checking, workspace
// carving and launch sequencing only — every byte of arithmetic happens in the gfx950 kernels of
// aid_gemm.hip / aid_attn.hip.  No allocation, no synchronisation, no exceptions.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "aid_kernels.hpp"

namespace {

thread_local char g_err[256] = "";
thread_local aid::AttnPlan g_attn_plan;            // of this thread's last attention call: g_variant points into it
thread_local const char* g_variant = "";
thread_local const char* g_gemm_variant = "";

int fail_hip(hipError_t e, const char* where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return AID_ERR_LAUNCH;
}

// ---- live timing (aid_profile_begin / aid_profile_end) -------------------------------------------
struct ProfRec {
    hipEvent_t t0, t1;
    char name[64];
    double flops, bytes, flops_exec;
};
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;                      // guards g_prof: launches of several host threads may be profiled at once
std::vector<ProfRec> g_prof;
unsigned g_prof_gen = 0;                   // bumped by aid_profile_begin (under g_prof_mu): a ProfScope that straddles a restart of the
                                           // recorder must not write into the NEW list's record that happens to sit at its index

struct ProfScope {          // records an event pair around one launch when profiling is on
    hipStream_t stream;
    bool on;
    size_t idx = 0;         // this launch's record (other threads may append while the launch is being issued)
    unsigned gen = 0;       // recorder generation the record belongs to
    ProfScope(hipStream_t s, const char* name, double flops, double bytes, double flops_exec = -1.0)
        : stream(s), on(g_prof_on.load(std::memory_order_relaxed)) {
        if (!on) return;
        ProfRec r;
        (void)hipEventCreate(&r.t0);
        (void)hipEventCreate(&r.t1);
        snprintf(r.name, sizeof(r.name), "%s", name);
        r.flops = flops;
        r.bytes = bytes;
        r.flops_exec = flops_exec < 0.0 ? flops : flops_exec;
        (void)hipEventRecord(r.t0, stream);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        idx = g_prof.size();
        gen = g_prof_gen;
        g_prof.push_back(r);
    }
    void rename(const char* name) {      // the kernel symbol is known only after the launcher picked an engine
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (gen == g_prof_gen && idx < g_prof.size()) snprintf(g_prof[idx].name, sizeof(g_prof[idx].name), "%s", name);
    }
    ~ProfScope() {
        if (!on) return;
        hipEvent_t t1 = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_prof_mu);
            if (gen == g_prof_gen && idx < g_prof.size()) t1 = g_prof[idx].t1;
        }
        if (t1) (void)hipEventRecord(t1, stream);
    }
};

// ---- tuning knobs (aid_kernels.hpp: enum Tune) -----------------------------------------------------
const char* const g_tune_names[aid::TUNE_COUNT] = {"GEMM_VARIANT", "GEMM_PP", "GEMM_TRI", "ATTN_NW", "ATTN_QB", "ATTN_PIPE",
                                                   "ATTN_RES", "ATTN_RES_CHUNKS", "ATTN_ORDER", "ATTN_V2", "CU_SHARE", "GEMM_RS", "ATTN_TX", "ATTN_TX_TILES", "GEMM_LS",
                                                   "GEMM_LR_PP"};
// Largest value a knob accepts.  Every accepted value selects between kernels / launch shapes that compute THE SAME RESULT (the parity
// suite runs under each of them); values beyond the range are refused by aid_set_tuning and ignored in the environment.  Development
// builds (tools/dev/Makefile) widen two ranges: the attention timing ablations (kernels that skip work, "results are garbage";
// -DAID_ABLATIONS) are ATTN_RES_CHUNKS > 100, the row-stationary GEMM's stamps / ablations (-DAID_RS_VARIANTS) GEMM_PP up to 7.
#if defined(AID_ABLATIONS)
const int g_tune_max[aid::TUNE_COUNT] = {31, 3, 1, 8, 2, 1, 1, 1000, 1, 1, 8, 1, 1, 64, 1, 2};
#elif defined(AID_RS_VARIANTS)
const int g_tune_max[aid::TUNE_COUNT] = {31, 7, 1, 8, 2, 1, 1, 64, 1, 1, 8, 1, 1, 64, 1, 2};
#else
const int g_tune_max[aid::TUNE_COUNT] = {31, 3, 1, 8, 2, 1, 1, 64, 1, 1, 8, 1, 1, 64, 1, 2};
#endif
struct TuneTable {
    std::atomic<int> v[aid::TUNE_COUNT];        // independent integers: a knob flipped by one thread is seen by the launches of all
    TuneTable() {                               // runs once, when the library is loaded
        for (int i = 0; i < aid::TUNE_COUNT; ++i) {
            char name[64];
            snprintf(name, sizeof(name), "AID_%s", g_tune_names[i]);
            const char* e = getenv(name);
            const int x = (e && *e) ? atoi(e) : -1;
            v[i].store((x < 0 || x > g_tune_max[i]) ? -1 : x, std::memory_order_relaxed);
        }
    }
};
TuneTable g_tune;

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }
inline bool dtype16(int d) { return d == AID_DTYPE_F16 || d == AID_DTYPE_BF16; }
inline bool dtype_ok(int d) { return dtype16(d) || d == AID_DTYPE_F32; }
inline const char* dtype_name(int d) { return d == AID_DTYPE_F16 ? "f16" : d == AID_DTYPE_BF16 ? "bf16" : "f32"; }

int check_problem(const AidGemmProblem& q) {
    if (!q.a || !q.b || !q.c) return AID_ERR_ARG;
    if (q.m < 0 || q.n < 0 || q.k <= 0 || q.batch < 1) return AID_ERR_ARG;
    if (q.k % 8 || q.lda % 8 || q.ldb % 8 || q.ldc % 4) return AID_ERR_SHAPE;
    if (q.lda < q.k || q.ldb < q.k || (!q.trans_rows && q.ldc < round_up(q.n, 4))) return AID_ERR_SHAPE;
    if (!aligned16(q.a) || !aligned16(q.b) || !aligned16(q.c)) return AID_ERR_SHAPE;
    if ((q.stride_a % 8) || (q.stride_b % 8) || (q.stride_c % 4)) return AID_ERR_SHAPE;
    if (q.trans_rows < 0) return AID_ERR_ARG;
    if (q.trans_rows) {                                  // C transposed per frame (aid_hip.h)
        if (q.batch != 1 || q.bias || q.residual || q.m % q.trans_rows || (q.ln_stats && q.ln_side != 1)) return AID_ERR_ARG;
        if (q.trans_rows % 8 || q.ldc % 8 || q.ldc < q.trans_rows || q.stride_c % 8) return AID_ERR_SHAPE;
    }
    if (q.lr_k < 0) return AID_ERR_ARG;
    if (q.lr_k > 0) {                                    // low-rank second K segment (ABI v9)
        if (!q.lr_a || !q.lr_b || q.ln_stats) return AID_ERR_ARG;      // the folded LayerNorm's correction would scale the term too
        if (q.lr_k % 64 || q.lr_k > 512 || q.lr_lda % 8 || q.lr_ldb % 8 || q.lr_lda < q.lr_k || q.lr_ldb < q.lr_k) return AID_ERR_SHAPE;
        if (q.lr_stride_a % 8 || q.lr_stride_b % 8 || !aligned16(q.lr_a) || !aligned16(q.lr_b)) return AID_ERR_SHAPE;
    }
    if (q.lr_row_scale) {                                // DoRA gain on the weight rows (ABI v10): part of the low-rank segment
        if (q.lr_k == 0 || (q.lr_scale_side != 1 && q.lr_scale_side != 2) || !aligned4(q.lr_row_scale)) return AID_ERR_ARG;
        if (q.trans_rows && q.lr_scale_side != 2) return AID_ERR_ARG;     // the flat value projection: the weight is b
    }
    if (q.f32_split != 0 && q.f32_split != 1) return AID_ERR_ARG;         // float32 matmul precision
    return AID_OK;
}

struct Carve {
    size_t q, k, vt, o, k2, vt2, xn, kip, vtip, ux, uctx, uo, ctab, total;
    int lp, tp;
    int rx, rctx;                                         // LoRA: columns of U of x / of ctx
};

// bytes of the pair table of a corner-weighted call (aid_hip.h): the INNER coefficient vector, then (coef_p, scale_p) per pass,
// n_frames floats each
size_t corner_table_bytes(int n_frames, int n_corners) {
    return align_up((size_t)(1 + 2 * ((n_corners + 1) / 2)) * n_frames * sizeof(float), 256);
}

// kv_extra: rows of k / V^T behind the projected ones (end-point store replay: the begin and the end frame's)
// corners: > 0 = a corner-weighted call among that many corners, whose pair table lies behind everything else
Carve carve(const AidProcessorArgs& a, int kv_extra = 0, int corners = 0) {
    Carve c;
    const size_t es = a.dtype == AID_DTYPE_F32 ? 4 : 2;
    const int nctx = a.ctx ? a.n_ctx : a.n_frames;
    const int l = a.ctx ? a.l : a.s;
    c.lp = round_up(l, 8);
    size_t off = 0;
    c.q = off;  off += align_up((size_t)a.n_frames * a.s * a.c * es, 256);
    c.k = off;  off += align_up((size_t)(nctx + kv_extra) * l * a.c * es, 256);
    c.vt = off; off += align_up((size_t)(nctx + kv_extra) * a.c * c.lp * es, 256);
    c.o = off;  off += align_up((size_t)a.n_frames * a.s * a.c * es, 256);
    c.k2 = c.vt2 = off;
    if (a.mode == AID_MODE_INNER) {                       // interpolated K / V^T, one row per frame
        c.k2 = off;  off += align_up((size_t)a.n_frames * l * a.c * es, 256);
        c.vt2 = off; off += align_up((size_t)a.n_frames * a.c * c.lp * es, 256);
    }
    c.xn = off;
    if (a.ln_eps > 0.f)                                   // LayerNorm(x), or only its row statistics when folded
        off += align_up(a.ln_wq ? (size_t)a.n_frames * a.s * 2 * sizeof(float) : (size_t)a.n_frames * a.s * a.c * es, 256);
    c.kip = c.vtip = off;
    c.tp = round_up(a.ip ? a.t_ip : 0, 8);
    if (a.ip) {                                           // image keys / values^T of the IP-Adapter branch
        c.kip = off;  off += align_up((size_t)a.n_ip * a.t_ip * a.c * es, 256);
        c.vtip = off; off += align_up((size_t)a.n_ip * a.c * c.tp * es, 256);
    }
    c.ux = c.uctx = c.uo = off;                           // LoRA: U = input A_pack^T of x (q [k v]), ctx (k v) and o
    c.rx = a.lora_r_q + (a.ctx ? 0 : a.lora_r_k + a.lora_r_v);
    c.rctx = a.ctx ? a.lora_r_k + a.lora_r_v : 0;
    if (c.rx) { c.ux = off; off += align_up((size_t)a.n_frames * a.s * c.rx * es, 256); }
    if (c.rctx) { c.uctx = off; off += align_up((size_t)a.n_ctx * a.l * c.rctx * es, 256); }
    if (a.lora_r_o) { c.uo = off; off += align_up((size_t)a.n_frames * a.s * a.lora_r_o * es, 256); }
    c.ctab = off;
    if (corners > 0) off += corner_table_bytes(a.n_frames, corners);
    c.total = off;
    return c;
}

// image segments of aid_ip_attn_fwd / aid_processor_ip_fwd (aid_hip.h): any count >= 1 here, the callers bound it
int check_ip_segments(const AidIpSegment* segs, int n, int n_frames) {
    if (!segs || n < 1) return AID_ERR_ARG;
    for (int g = 0; g < n; ++g) {
        const AidIpSegment& s = segs[g];
        if (!s.k || !s.vt || s.t < 1 || (s.n_rows != 1 && s.n_rows != n_frames)) return AID_ERR_ARG;
        if (s.ldvt % 8 || s.ldvt < s.t || s.k_fs % 8 || s.vt_fs % 8 || s.k_fs < 0 || s.vt_fs < 0) return AID_ERR_SHAPE;
        if (!aligned16(s.k) || !aligned16(s.vt) || (s.row_weight && !aligned4(s.row_weight))) return AID_ERR_SHAPE;
    }
    return AID_OK;
}

int check_processor(const AidProcessorArgs& a) {
    if (!a.x || !a.wq || !a.wk || !a.wv || !a.wo || !a.y) return AID_ERR_ARG;
    if (!dtype_ok(a.dtype)) return AID_ERR_DTYPE;
    if (a.dtype == AID_DTYPE_F32 && a.ln_eps > 0.f) return AID_ERR_DTYPE;      // the LayerNorm fusion is 16-bit only
    if (a.n_frames < 1 || a.s < 1 || a.c < 1 || a.heads < 1 || a.c % a.heads) return AID_ERR_ARG;
    if (a.mode < AID_MODE_PLAIN || a.mode > AID_MODE_OUTER) return AID_ERR_ARG;
    if (a.mode != AID_MODE_PLAIN && !a.coef) return AID_ERR_ARG;
    if (!aid::attn_head_dim_supported(a.c / a.heads)) return AID_ERR_SHAPE;
    if (a.c % 8) return AID_ERR_SHAPE;
    const int nctx = a.ctx ? a.n_ctx : a.n_frames;
    if (a.ctx) {
        if (a.l < 1 || a.cc < 8 || a.cc % 8 || a.n_ctx < 1) return AID_ERR_ARG;
        if (!a.ctx_map && a.n_ctx != a.n_frames) return AID_ERR_ARG;
    } else if (a.ctx_map) {
        return AID_ERR_ARG;
    }
    if (a.mode != AID_MODE_PLAIN && (a.begin < 0 || a.begin >= nctx || a.end < 0 || a.end >= nctx)) return AID_ERR_ARG;
    if (a.ip) {
        if (!a.ctx || !a.wk_ip || !a.wv_ip || a.n_ip < 1 || a.t_ip < 1) return AID_ERR_ARG;
        if (a.ip_mode != AID_IP_SAME && a.ip_mode != AID_IP_PLAIN) return AID_ERR_ARG;
        if (a.ip_mode == AID_IP_SAME && (a.mode != AID_MODE_OUTER || a.ip_begin < 0 || a.ip_begin >= a.n_ip ||
                                         a.ip_end < 0 || a.ip_end >= a.n_ip)) return AID_ERR_ARG;
        if (!a.ip_map && a.n_ip < a.n_frames) return AID_ERR_ARG;
        if (a.ip_stride % 8 || a.ip_stride < (int64_t)a.t_ip * a.cc) return AID_ERR_SHAPE;
        if (!aligned16(a.ip) || !aligned16(a.wk_ip) || !aligned16(a.wv_ip)) return AID_ERR_SHAPE;
    } else if (a.ip_mode != AID_IP_NONE) {
        return AID_ERR_ARG;
    }
    if ((a.k_cached != nullptr) != (a.vt_cached != nullptr)) return AID_ERR_ARG;
    if (a.k_cached && (!a.ctx || !aligned16(a.k_cached) || !aligned16(a.vt_cached))) return AID_ERR_ARG;
    if (a.attn_bias && ((a.fused && a.mode != AID_MODE_PLAIN) || a.ip || a.attn_bias_fs < 0 || a.attn_bias_hs < 0 || a.attn_bias_rs < 0))
        return AID_ERR_ARG;                            // the mask covers one key segment (aid_hip.h); the image branch has no mask to take
    if (!(a.ln_eps >= 0.f) || a.cu_share < 0 || a.cu_share > 8) return AID_ERR_ARG;
    if ((a.f32_split != 0 && a.f32_split != 1) || (a.f32_split && a.dtype != AID_DTYPE_F32)) return AID_ERR_ARG;
    if ((a.f32_attn_split != 0 && a.f32_attn_split != 1) || (a.f32_attn_split && a.dtype != AID_DTYPE_F32)) return AID_ERR_ARG;
    if (a.ln_eps > 0.f) {
        if (!aid::layernorm_width_supported(a.c)) return AID_ERR_SHAPE;
        if ((a.ln_gamma && !aligned16(a.ln_gamma)) || (a.ln_beta && !aligned16(a.ln_beta))) return AID_ERR_SHAPE;
        if (a.ln_wq) {                              // folded: the projections run on x itself with pre-multiplied weights
            if (!a.ln_const || a.c % 64 || !aligned16(a.ln_wq)) return AID_ERR_SHAPE;
            if (!a.ctx && (!a.ln_wk || !a.ln_wv || !aligned16(a.ln_wk) || !aligned16(a.ln_wv))) return AID_ERR_ARG;
        }
    }
    // LoRA (ABI v9): ranks are multiples of 64 up to 512; every projection with a rank needs its up weights and its stacked down weights
    const int32_t ranks[4] = {a.lora_r_q, a.lora_r_k, a.lora_r_v, a.lora_r_o};
    const void* ups[4] = {a.lora_up_q, a.lora_up_k, a.lora_up_v, a.lora_up_o};
    bool any = false;
    for (int i = 0; i < 4; ++i) {
        if (ranks[i] < 0) return AID_ERR_ARG;
        if (!ranks[i]) continue;
        any = true;
        if (ranks[i] % 64 || ranks[i] > 512) return AID_ERR_SHAPE;
        if (!ups[i] || !aligned16(ups[i])) return AID_ERR_ARG;
    }
    const float* gains[4] = {a.lora_gain_q, a.lora_gain_k, a.lora_gain_v, a.lora_gain_o};      // DoRA (ABI v10): only with a rank
    for (int i = 0; i < 4; ++i)
        if (gains[i] && (!ranks[i] || !aligned4(gains[i]))) return AID_ERR_ARG;
    if (any) {
        if (a.ln_wq) return AID_ERR_ARG;            // the folded LayerNorm's correction would scale the low-rank term too
        if (a.k_cached && (a.lora_r_k || a.lora_r_v)) return AID_ERR_ARG;     // cached keys must already hold the adapter term
        const bool need_x = a.lora_r_q || (!a.ctx && (a.lora_r_k || a.lora_r_v));
        const bool need_ctx = a.ctx && (a.lora_r_k || a.lora_r_v);
        if ((need_x && (!a.lora_down_x || !aligned16(a.lora_down_x))) || (need_ctx && (!a.lora_down_ctx || !aligned16(a.lora_down_ctx))) ||
            (a.lora_r_o && (!a.lora_down_o || !aligned16(a.lora_down_o))))
            return AID_ERR_ARG;
    }
    return AID_OK;
}

}  // namespace

namespace aid {
int tune(int id) { return (id >= 0 && id < TUNE_COUNT) ? g_tune.v[id].load(std::memory_order_relaxed) : -1; }
}  // namespace aid

extern "C" {

int aid_abi_version(void) { return AID_ABI_VERSION; }

int aid_set_tuning(const char* name, int value) {
    if (!name) return AID_ERR_ARG;
    if (!strncmp(name, "AID_", 4)) name += 4;
    for (int i = 0; i < aid::TUNE_COUNT; ++i)
        if (!strcmp(name, g_tune_names[i])) {
            if (value > g_tune_max[i]) return AID_ERR_ARG;      // no value may change results (see g_tune_max)
            g_tune.v[i].store(value < 0 ? -1 : value, std::memory_order_relaxed);
            return AID_OK;
        }
    return AID_ERR_ARG;
}

int aid_get_tuning(const char* name, int* value) {
    if (!name || !value) return AID_ERR_ARG;
    if (!strncmp(name, "AID_", 4)) name += 4;
    for (int i = 0; i < aid::TUNE_COUNT; ++i)
        if (!strcmp(name, g_tune_names[i])) {
            *value = g_tune.v[i].load(std::memory_order_relaxed);
            return AID_OK;
        }
    return AID_ERR_ARG;
}

const char* aid_strerror(int code) {
    switch (code) {
        case AID_OK: return "ok";
        case AID_ERR_ARG: return "invalid argument (NULL pointer, negative size or inconsistent field)";
        case AID_ERR_DTYPE: return "unsupported dtype (AID_DTYPE_F16 / _BF16 / _F32; the LayerNorm entry points and the ln_* options of aid_processor_fwd are 16-bit only)";
        case AID_ERR_SHAPE: return "unsupported shape or alignment (head dim must be 40/64/80/160; see aid_hip.h)";
        case AID_ERR_WORKSPACE: return "workspace too small or misaligned";
        case AID_ERR_LAUNCH: return g_err[0] ? g_err : "kernel launch failed";
        case AID_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown error code";
    }
}

const char* aid_last_attn_variant(void) { return g_variant; }
const char* aid_last_gemm_variant(void) { return g_gemm_variant; }

int aid_device_info(int* n_cu, int* clock_khz, char* arch) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AID_ERR_NO_DEVICE;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return AID_ERR_NO_DEVICE;
    if (n_cu) *n_cu = pr.multiProcessorCount;
    if (clock_khz) *clock_khz = pr.clockRate;
    if (arch) { strncpy(arch, pr.gcnArchName, 31); arch[31] = 0; }
    return AID_OK;
}

int aid_stream_capture_id(void* stream, unsigned long long* id) {
    if (!id) return AID_ERR_ARG;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    const hipError_t e = hipStreamGetCaptureInfo(static_cast<hipStream_t>(stream), &st, &cid);
    if (e != hipSuccess) return fail_hip(e, "aid_stream_capture_id");
    *id = st == hipStreamCaptureStatusActive ? cid : 0ull;
    return AID_OK;
}

int aid_profile_begin(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.t0); (void)hipEventDestroy(r.t1); }
    g_prof.clear();
    ++g_prof_gen;
    g_prof_on.store(true);
    return AID_OK;
}

int aid_profile_end(AidProfileEntry* entries, int max_entries) {
    g_prof_on.store(false);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = 0;
    int rc = AID_OK;
    for (auto& r : g_prof) {
        hipError_t e = hipEventSynchronize(r.t1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.t0, r.t1);
        if (e != hipSuccess) rc = fail_hip(e, "aid_profile_end");
        if (entries && n < max_entries && e == hipSuccess) {
            memcpy(entries[n].kernel, r.name, sizeof(r.name));
            entries[n].ms = ms;
            entries[n].flops = r.flops;
            entries[n].bytes = r.bytes;
            entries[n].flops_executed = r.flops_exec;
            ++n;
        }
        (void)hipEventDestroy(r.t0);
        (void)hipEventDestroy(r.t1);
    }
    g_prof.clear();
    return rc == AID_OK ? n : rc;
}

int aid_gemm_nt(const AidGemmProblem* problems, int n_problems, int dtype, void* stream) {
    if (!problems || n_problems < 1 || n_problems > AID_GEMM_MAX_PROBLEMS) return AID_ERR_ARG;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (problems[0].cu_share < 0 || problems[0].cu_share > 8) return AID_ERR_ARG;
    aid::GemmGroup g;
    memset(&g, 0, sizeof(g));
    g.n_problems = n_problems;
    aid::GemmLR lr;
    memset(&lr, 0, sizeof(lr));
    bool has_lr = false;
    // float32 matmul precision "high" (f32_split) is a permission: the split kernel runs a group only if every problem grants it and the
    // group is plain (that kernel carries neither the low-rank segment nor the folded LayerNorm); every other group runs exact
    bool split = dtype == AID_DTYPE_F32;
    for (int i = 0; i < n_problems; ++i) {
        const AidGemmProblem& q = problems[i];
        int rc = check_problem(q);
        if (rc != AID_OK) return rc;
        if (q.f32_split && dtype != AID_DTYPE_F32) return AID_ERR_ARG;
        if (!q.f32_split || q.ln_stats || q.lr_k > 0) split = false;
        if (q.lr_k > 0) {
            aid::GemmLRDesc& L = lr.p[i];
            L.a = q.lr_a; L.b = q.lr_b; L.k = q.lr_k; L.lda = q.lr_lda; L.ldb = q.lr_ldb;
            L.stride_a = q.lr_stride_a; L.stride_b = q.lr_stride_b;
            L.row_scale = q.lr_row_scale; L.side = q.lr_scale_side;
            has_lr = true;
        }
        aid::GemmDesc& d = g.p[i];
        d.a = q.a; d.b = q.b; d.c = q.c; d.bias = q.bias; d.residual = q.residual;
        d.m = q.m; d.n = q.n; d.k = q.k;
        d.lda = q.lda; d.ldb = q.ldb; d.ldc = q.ldc;
        d.batch = q.batch;
        d.scale = q.scale == 0.f ? 1.f : q.scale;
        d.stride_a = q.stride_a; d.stride_b = q.stride_b; d.stride_c = q.stride_c;
        d.trans_rows = q.trans_rows;
        if (q.ln_stats) {
            if (!q.ln_colsum || !q.ln_shift || (q.ln_side != 1 && q.ln_side != 2) || q.stride_stats < 0) return AID_ERR_ARG;
            d.ln_stats = q.ln_stats; d.ln_colsum = q.ln_colsum; d.ln_shift = q.ln_shift;
            d.ln_side = q.ln_side; d.stride_stats = q.stride_stats;
        }
    }
    double flops = 0, bytes = 0;
    if (g_prof_on.load(std::memory_order_relaxed)) {
        for (int i = 0; i < n_problems; ++i) {
            const AidGemmProblem& q = problems[i];
            flops += 2.0 * q.m * q.n * ((double)q.k + q.lr_k) * q.batch;
            bytes += 2.0 * ((double)q.m * q.k * (q.stride_a || q.batch == 1 ? q.batch : 1) +
                            (double)q.n * q.k * (q.stride_b || q.batch == 1 ? q.batch : 1) +
                            (double)q.m * q.n * q.batch * (q.residual ? 2 : 1));
            if (q.lr_k > 0)
                bytes += 2.0 * ((double)q.m * q.lr_k * (q.lr_stride_a || q.batch == 1 ? q.batch : 1) +
                                (double)q.n * q.lr_k * (q.lr_stride_b || q.batch == 1 ? q.batch : 1));
            if (q.lr_row_scale) bytes += 4.0 * (q.lr_scale_side == 1 ? q.m : q.n);
        }
    }
    hipError_t e;
    {
        ProfScope ps(static_cast<hipStream_t>(stream), "aid_gemm_nt", flops, dtype == AID_DTYPE_F32 ? 2.0 * bytes : bytes);
        if (split) {
            e = aid::gemm_f32x3_launch(g, static_cast<hipStream_t>(stream));
            g_gemm_variant = "f32x3";
            ps.rename("aid_gemm_f32x3_kernel");
        } else if (dtype == AID_DTYPE_F32) {
            e = aid::gemm_f32_launch(g, static_cast<hipStream_t>(stream), has_lr ? &lr : nullptr);
            g_gemm_variant = "f32";
            ps.rename(has_lr ? "aid_gemm_f32_kernel_lr" : "aid_gemm_f32_kernel");
        } else {
            // profile entries carry the kernel SYMBOL that ran, so they line up with rocprofv3's per-kernel rows; `_lr` (here and in
            // the fp32 label above) names the GemmLR instantiation of the kernel, which rocprofv3 prints as `...kernel<..., aid::GemmLR>`
            const char* sym = "aid_gemm_nt_kernel";
            e = aid::gemm_group_launch(g, dtype, static_cast<hipStream_t>(stream), &g_gemm_variant, &sym, problems[0].cu_share,
                                       has_lr ? &lr : nullptr);
            char nm[64];
            snprintf(nm, sizeof(nm), "%s<%s>", sym, dtype_name(dtype));
            ps.rename(nm);
        }
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_gemm_nt");
}

int aid_layernorm(const void* x, const void* gamma, const void* beta, void* y, int64_t rows, int32_t c, float eps,
                  int32_t dtype, void* stream) {
    if (!x || !y || rows < 0 || !(eps >= 0.f)) return AID_ERR_ARG;
    if (dtype != AID_DTYPE_F16 && dtype != AID_DTYPE_BF16) return AID_ERR_DTYPE;
    if (!aid::layernorm_width_supported(c)) return AID_ERR_SHAPE;
    if (!aligned16(x) || !aligned16(y) || (gamma && !aligned16(gamma)) || (beta && !aligned16(beta))) return AID_ERR_SHAPE;
    hipError_t e;
    {
        ProfScope ps(static_cast<hipStream_t>(stream), dtype == AID_DTYPE_F16 ? "aid_layernorm<f16>" : "aid_layernorm<bf16>",
                     8.0 * rows * c, 4.0 * rows * c);
        e = aid::layernorm_launch(x, gamma, beta, y, rows, c, eps, dtype, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_layernorm");
}

int aid_ln_stats(const void* x, float* stats, int64_t rows, int32_t c, float eps, int32_t dtype, void* stream) {
    if (!x || !stats || rows < 0 || !(eps >= 0.f)) return AID_ERR_ARG;
    if (dtype != AID_DTYPE_F16 && dtype != AID_DTYPE_BF16) return AID_ERR_DTYPE;
    if (!aid::layernorm_width_supported(c) || !aligned16(x)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        ProfScope ps(static_cast<hipStream_t>(stream), dtype == AID_DTYPE_F16 ? "aid_ln_stats<f16>" : "aid_ln_stats<bf16>",
                     4.0 * rows * c, 2.0 * rows * c + 8.0 * rows);
        e = aid::ln_stats_launch(x, stats, rows, c, eps, dtype, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_ln_stats");
}

int aid_ln_fold(const void* w, const void* gamma, const void* beta, void* w_folded, float* colsum, float* shift,
                int32_t rows, int32_t c, int32_t dtype, void* stream) {
    if (!w || !w_folded || !colsum || !shift || rows < 1) return AID_ERR_ARG;
    if (dtype != AID_DTYPE_F16 && dtype != AID_DTYPE_BF16) return AID_ERR_DTYPE;
    if (!aid::layernorm_width_supported(c)) return AID_ERR_SHAPE;
    if (!aligned16(w) || !aligned16(w_folded) || (gamma && !aligned16(gamma)) || (beta && !aligned16(beta))) return AID_ERR_SHAPE;
    const hipError_t e = aid::ln_fold_launch(w, gamma, beta, w_folded, colsum, shift, rows, c, dtype,
                                             static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_ln_fold");
}

int aid_dora_gain(const void* w, const void* a_pack, const void* b_pack, const void* magnitude, float* gain, int32_t n_out,
                  int32_t n_in, int32_t ldw, int32_t rank, int32_t dtype, void* stream) {
    if (!w || !a_pack || !b_pack || !magnitude || !gain || n_out < 0 || n_in < 1 || rank < 1 || !aligned4(gain)) return AID_ERR_ARG;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (n_in % 8 || ldw % 8 || ldw < n_in || rank % 64 || rank > 512) return AID_ERR_SHAPE;
    if (!aligned16(w) || !aligned16(a_pack) || !aligned16(b_pack) || !aligned16(magnitude)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        // traffic: W, B_pack and the magnitude once, A_pack once per row group (from L2), the gain written
        const double es = dtype == AID_DTYPE_F32 ? 4.0 : 2.0;
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_dora_gain<%s>", dtype_name(dtype));
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 2.0 * n_out * (double)n_in * (rank + 1),
                     es * ((double)n_out * n_in + (double)rank * n_in + (double)n_out * rank + n_out) + 4.0 * n_out);
        e = aid::dora_gain_launch(w, a_pack, b_pack, magnitude, gain, n_out, n_in, ldw, rank, dtype, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_dora_gain");
}

int aid_cfg_rescale(const void* text, const void* uncond, void* out, int32_t n, int64_t e, int64_t text_stride, int64_t uncond_stride,
                    int64_t out_stride, float guidance_scale, float guidance_rescale, int32_t dtype, void* stream) {
    if (!text || !uncond || !out || n < 0) return AID_ERR_ARG;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (e < 2) return AID_ERR_SHAPE;                                   // the unbiased std of one element is undefined
    if (text_stride < e || uncond_stride < e || out_stride < e) return AID_ERR_ARG;
    if (!(guidance_rescale >= 0.f && guidance_rescale <= 1.f)) return AID_ERR_ARG;
    const int64_t es = dtype == AID_DTYPE_F32 ? 4 : 2;
    const uintptr_t pt = reinterpret_cast<uintptr_t>(text), pu = reinterpret_cast<uintptr_t>(uncond), po = reinterpret_cast<uintptr_t>(out);
    if ((pt | pu | po) % es) return AID_ERR_SHAPE;                     // (strides are in elements: every sample is aligned with its base)
    if (n > 0) {
        // out may BE an input (same base, same stride: every element is read before the same lane writes it); any other overlap of
        // the bytes the call writes with the bytes it reads is refused
        const uintptr_t in_p[2] = {pt, pu};
        const int64_t in_s[2] = {text_stride, uncond_stride};
        const uintptr_t o_end = po + (uintptr_t)(((int64_t)(n - 1) * out_stride + e) * es);
        for (int i = 0; i < 2; ++i) {
            if (in_p[i] == po && in_s[i] == out_stride) continue;
            const uintptr_t i_end = in_p[i] + (uintptr_t)(((int64_t)(n - 1) * in_s[i] + e) * es);
            if (po < i_end && in_p[i] < o_end) return AID_ERR_ARG;
        }
    }
    if (n == 0) return AID_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AID_ERR_NO_DEVICE;
    hipError_t err;
    {
        // traffic: text and uncond read, out written (the second and third walk of a sample hit L2)
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_cfg_rescale<%s>", dtype_name(dtype));
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 12.0 * n * (double)e, 3.0 * es * n * (double)e);
        err = aid::cfg_rescale_launch(text, uncond, out, n, e, text_stride, uncond_stride, out_stride, guidance_scale, guidance_rescale,
                                      dtype, static_cast<hipStream_t>(stream));
    }
    return err == hipSuccess ? AID_OK : fail_hip(err, "aid_cfg_rescale");
}

// everything aid_attn_fwd refuses (aid_hip.h), before any launch
static int check_attn(const AidAttnArgs& a) {
    if (!a.q || !a.k || !a.vt || !a.out) return AID_ERR_ARG;
    if (!dtype_ok(a.dtype)) return AID_ERR_DTYPE;
    if (a.mode < AID_MODE_PLAIN || a.mode > AID_MODE_OUTER) return AID_ERR_ARG;
    if (a.n_frames < 1 || a.n_kv < 1 || a.s < 1 || a.l < 1 || a.heads < 1) return AID_ERR_ARG;
    if (a.mode != AID_MODE_PLAIN && (!a.coef || a.begin < 0 || a.begin >= a.n_kv || a.end < 0 || a.end >= a.n_kv))
        return AID_ERR_ARG;
    if (!a.kv_map && a.n_kv < a.n_frames) return AID_ERR_ARG;
    if (a.mode == AID_MODE_INNER && (!a.k2 || !a.vt2 || !aligned16(a.k2) || !aligned16(a.vt2))) return AID_ERR_ARG;
    if ((a.f32_split != 0 && a.f32_split != 1) || (a.f32_split && a.dtype != AID_DTYPE_F32)) return AID_ERR_ARG;   // precision of the two products
    if (!aid::attn_head_dim_supported(a.d)) return AID_ERR_SHAPE;
    if (a.ldq % 8 || a.ldk % 8 || a.ldvt % 8 || a.ldo % 4 || a.ldvt < a.l) return AID_ERR_SHAPE;
    if (a.q_fs % 8 || a.k_fs % 8 || a.vt_fs % 8 || a.o_fs % 4) return AID_ERR_SHAPE;
    if (!aligned16(a.q) || !aligned16(a.k) || !aligned16(a.vt) || !aligned16(a.out)) return AID_ERR_SHAPE;
    if (a.bias) {
        // one mask row covers ONE segment of l keys: the reference's fused calls fail at the broadcast of the l-wide mask against the
        // 2 l scores of [own ; end-point] keys (interpolation.py:644-651), so there is nothing to be equal to
        if (a.fused && a.mode != AID_MODE_PLAIN) return AID_ERR_ARG;
        if (a.bias_fs < 0 || a.bias_hs < 0 || a.bias_rs < 0) return AID_ERR_ARG;
        if (reinterpret_cast<uintptr_t>(a.bias) % (a.dtype == AID_DTYPE_F32 ? 4 : 2)) return AID_ERR_SHAPE;
    }
    return AID_OK;
}

int aid_attn_fwd(const AidAttnArgs* args, void* stream) {
    if (!args) return AID_ERR_ARG;
    const AidAttnArgs& a = *args;
    const int chk = check_attn(a);
    if (chk != AID_OK) return chk;
    // algorithmic work: key segments per frame — plain 1, pure inner 1, fused inner 2,
    // pure outer 2, fused outer 3
    const int segs = a.mode == AID_MODE_PLAIN ? 1 : (a.mode == AID_MODE_INNER ? 1 : 2) + (a.fused ? 1 : 0);
    const double c = (double)a.heads * a.d;
    const double per_seg = 4.0 * a.s * (double)a.l * c;
    const double flops = per_seg * ((double)segs * (a.n_frames - a.n_plain) + a.n_plain);
    const double flops_exec = a.seg_executed > 0 ? per_seg * a.seg_executed : flops;
    const double bytes = (a.dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * (2.0 * a.n_frames * a.s * c + 2.0 * a.n_kv * a.l * c);
    // which kernel(s), their names and their shares of the call: aid::plan_attn (aid_attn.hip).  A split call is two launches: the
    // frames with one key segment (one segment's work each, all of it executed), then the rest of the call's work on the other frames.
    const aid::AttnPlan& pl = g_attn_plan = aid::plan_attn(a);
    const double f_single = per_seg * pl.n_single;
    const struct { double flops, bytes, flops_exec; } work[3] = {        // indexed by aid::AttnShare
        {flops, bytes, flops_exec},
        {f_single, bytes * pl.n_single / a.n_frames, f_single},
        {flops - f_single, bytes * (a.n_frames - pl.n_single) / a.n_frames, flops_exec - f_single}};
    hipError_t e = hipSuccess;
    for (int i = 0; i < pl.n_steps && e == hipSuccess; ++i) {
        const aid::AttnStep& st = pl.step[i];
        const auto& w = work[static_cast<int>(st.share)];
        ProfScope ps(static_cast<hipStream_t>(stream), st.label, w.flops, w.bytes, w.flops_exec);
        e = aid::launch_attn_plan(a, st, static_cast<hipStream_t>(stream));
    }
    g_variant = pl.variant;
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_attn_fwd");
}

int aid_ip_attn_fwd(const AidIpAttnArgs* args, void* stream) {
    if (!args) return AID_ERR_ARG;
    const AidIpAttnArgs& a = *args;
    if (!a.q || !a.out || !a.segments) return AID_ERR_ARG;
    if (a.n_segments < 1 || a.n_segments > AID_IP_MAX_SEGMENTS) return AID_ERR_ARG;
    if (a.n_frames < 1 || a.s < 1 || a.heads < 1 || a.d < 1) return AID_ERR_ARG;
    if (!a.q_prescaled && !(a.softmax_scale > 0.f)) return AID_ERR_ARG;
    if (!dtype16(a.dtype)) return AID_ERR_DTYPE;            // float32 storage has no segment form
    if (!aid::attn_head_dim_supported(a.d)) return AID_ERR_SHAPE;
    if (a.ldq % 8 || a.ldo % 8 || a.q_fs % 8 || a.o_fs % 8 || a.q_fs < 0 || a.o_fs < 0) return AID_ERR_SHAPE;
    if ((int64_t)a.ldq < (int64_t)a.heads * a.d || (int64_t)a.ldo < (int64_t)a.heads * a.d) return AID_ERR_SHAPE;
    if (!aligned16(a.q) || !aligned16(a.out)) return AID_ERR_SHAPE;
    const int rc = check_ip_segments(a.segments, a.n_segments, a.n_frames);
    if (rc != AID_OK) return rc;
    hipError_t e;
    {
        // work: 4 s t c per (frame, segment); traffic: q read, out read and written, every segment's K / V^T rows once
        const double c = (double)a.heads * a.d;
        double keys = 0, kv = 0;
        for (int g = 0; g < a.n_segments; ++g) {
            keys += a.segments[g].t;
            kv += 2.0 * a.segments[g].n_rows * (double)a.segments[g].t * c;
        }
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_ip_attn<%s,d%d,g%d>", dtype_name(a.dtype), a.d, a.n_segments);
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 4.0 * a.n_frames * a.s * keys * c, 2.0 * (3.0 * a.n_frames * a.s * c + kv));
        e = aid::ip_attn_launch(a, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_ip_attn_fwd");
}

static int lerp_kv_impl(const void* k, const void* vt, void* k2, void* vt2, const float* coef, int32_t n_frames,
                        int32_t begin, int32_t end, int64_t k_fs, int64_t vt_fs, int32_t dtype, void* stream,
                        int n_interior) {
    if (!k || !vt || !k2 || !vt2 || !coef || n_frames < 1 || begin < 0 || end < 0) return AID_ERR_ARG;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (k_fs % 8 || vt_fs % 8 || !aligned16(k) || !aligned16(vt) || !aligned16(k2) || !aligned16(vt2)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        // algorithmic traffic: the two end-point frames read once, one interpolated row written per interior frame
        const double elems = (double)(k_fs + vt_fs);
        ProfScope ps(static_cast<hipStream_t>(stream), dtype == AID_DTYPE_F16 ? "aid_lerp_kv<f16>" : dtype == AID_DTYPE_BF16 ? "aid_lerp_kv<bf16>" : "aid_lerp_kv<f32>",
                     3.0 * n_interior * elems, (dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * (2.0 + n_interior) * elems);
        if (dtype == AID_DTYPE_F32)
            e = aid::lerp_kv_f32_launch(k, vt, k2, vt2, coef, n_frames, begin, end, k_fs, vt_fs, static_cast<hipStream_t>(stream));
        else
            e = aid::lerp_kv_launch(k, vt, k2, vt2, coef, n_frames, begin, end, k_fs, vt_fs, dtype,
                                    static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_lerp_kv");
}

int aid_lerp_kv(const void* k, const void* vt, void* k2, void* vt2, const float* coef, int32_t n_frames, int32_t begin,
                int32_t end, int64_t k_fs, int64_t vt_fs, int32_t dtype, void* stream) {
    return lerp_kv_impl(k, vt, k2, vt2, coef, n_frames, begin, end, k_fs, vt_fs, dtype, stream,
                        n_frames > 2 ? n_frames - 2 : 0);
}

// ---- corner-weighted AID (aid_hip.h) ---------------------------------------------------------------------------------------------
static int check_mix(const void* k, const void* vt, const void* k2, const void* vt2, const int32_t* rows, const float* weights,
                     int32_t n_frames, int32_t n_plain, int32_t n_corners, int64_t k_fs, int64_t vt_fs, int32_t dtype) {
    if (!k || !vt || !k2 || !vt2 || !rows || !weights) return AID_ERR_ARG;
    if (n_corners < 1 || n_corners > AID_MAX_CORNERS || n_frames < 1 || n_plain < 0 || n_plain > n_frames) return AID_ERR_ARG;
    for (int m = 0; m < n_corners; ++m)
        if (rows[m] < 0) return AID_ERR_ARG;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (k_fs < 8 || vt_fs < 8 || k_fs % 8 || vt_fs % 8) return AID_ERR_SHAPE;
    if (!aligned16(k) || !aligned16(vt) || !aligned16(k2) || !aligned16(vt2) || !aligned4(weights)) return AID_ERR_SHAPE;
    return AID_OK;
}

static int mix_kv_impl(const void* k, const void* vt, void* k2, void* vt2, const int32_t* rows, const float* weights, int32_t n_frames,
                       int32_t n_plain, int32_t n_corners, int64_t k_fs, int64_t vt_fs, int32_t dtype, void* stream) {
    aid::CornerRows cr;
    for (int m = 0; m < AID_MAX_CORNERS; ++m) cr.row[m] = rows[m < n_corners ? m : 0];
    const int n_mix = n_frames - n_plain;
    hipError_t e;
    {
        // traffic: the corner rows read once, one mixed row written per AID frame
        const double elems = (double)(k_fs + vt_fs);
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_mix_kv<%s,m%d>", dtype_name(dtype), n_corners);
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 2.0 * n_corners * n_mix * elems,
                     (dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * ((double)n_corners + n_mix) * elems);
        e = aid::mix_kv_launch(k, vt, k2, vt2, weights, cr, n_corners, n_mix, k_fs, vt_fs, dtype, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_mix_kv");
}

int aid_mix_kv(const void* k, const void* vt, void* k2, void* vt2, const int32_t* rows, const float* weights, int32_t n_frames,
               int32_t n_plain, int32_t n_corners, int64_t k_fs, int64_t vt_fs, int32_t dtype, void* stream) {
    const int rc = check_mix(k, vt, k2, vt2, rows, weights, n_frames, n_plain, n_corners, k_fs, vt_fs, dtype);
    if (rc != AID_OK) return rc;
    return mix_kv_impl(k, vt, k2, vt2, rows, weights, n_frames, n_plain, n_corners, k_fs, vt_fs, dtype, stream);
}

size_t aid_corners_scratch_bytes(int32_t n_frames, int32_t n_corners) {
    if (n_frames < 1 || n_corners < 1 || n_corners > AID_MAX_CORNERS) return 0;
    return corner_table_bytes(n_frames, n_corners);
}

// the AidCorners of a call over n_kv rows of k / V^T; `own_scratch`: the call brings the pair table's memory (aid_attn_corners_fwd)
static int check_corners(const AidCorners& c, int n_frames, int n_kv, int n_plain, bool own_scratch) {
    if (!c.rows || !c.weights || c.n_corners < 1 || c.n_corners > AID_MAX_CORNERS) return AID_ERR_ARG;
    if (n_plain < 0 || n_plain > n_frames) return AID_ERR_ARG;
    for (int m = 0; m < c.n_corners; ++m)
        if (c.rows[m] < 0 || c.rows[m] >= n_kv) return AID_ERR_ARG;
    if (!aligned4(c.weights)) return AID_ERR_SHAPE;
    if (own_scratch) {
        if (!c.scratch) return AID_ERR_ARG;
        if (!aligned16(c.scratch)) return AID_ERR_SHAPE;
        if (n_frames >= 1 && c.scratch_bytes < corner_table_bytes(n_frames, c.n_corners)) return AID_ERR_WORKSPACE;
    }
    return AID_OK;
}

// pass 0 of the composition as aid_attn_fwd sees it: what the checks of a corner call run on
static AidAttnArgs corner_pass0(const AidAttnArgs& a, const AidCorners& c, const float* tab) {
    AidAttnArgs at = a;
    const bool outer = a.mode == AID_MODE_OUTER;
    at.coef = outer ? tab + a.n_frames : tab;
    at.frame_scale = outer ? tab + 2 * (size_t)a.n_frames : nullptr;
    at.begin = c.rows[0];
    at.end = outer && c.n_corners > 1 ? c.rows[1] : c.rows[0];
    at.accumulate = 0;
    at.out_scale = 1.f;
    at.seg_executed = 0;
    return at;
}

// ---- key-frame blend (aid_hip.h): the corners are block rows of key-frame stores ---------------------------------------------------
// what is wrong with the AidKeyframeBlend itself, in two rounds so that a caller can keep the order ARG, DTYPE, SHAPE of every entry
static int check_blend_arg(const AidKeyframeBlend* b, int n_frames, int n_plain) {
    if (!b || !b->rows || !b->step || !b->weights || !aligned4(b->step)) return AID_ERR_ARG;
    if (b->n_corners < 1 || b->n_corners > AID_MAX_CORNERS || b->n_steps < 1 || (b->q8 != 0 && b->q8 != 1)) return AID_ERR_ARG;
    if (n_plain < 0 || n_plain > n_frames) return AID_ERR_ARG;
    for (int m = 0; m < b->n_corners; ++m)
        if (!b->rows[m].k_store || !b->rows[m].vt_store) return AID_ERR_ARG;
    return AID_OK;
}

static int check_blend_shape(const AidKeyframeBlend& b) {
    for (int m = 0; m < b.n_corners; ++m)
        if (!aligned16(b.rows[m].k_store) || !aligned16(b.rows[m].vt_store)) return AID_ERR_SHAPE;
    return aligned4(b.weights) ? AID_OK : AID_ERR_SHAPE;
}

static int check_mix_stores(const AidKeyframeBlend* b, const void* k2, const void* vt2, int32_t n_frames, int32_t n_plain, int64_t k_fs,
                            int64_t vt_fs, int32_t vt_ld, int32_t vt_cols, int32_t dtype) {
    if (!k2 || !vt2 || n_frames < 1) return AID_ERR_ARG;
    const int rc = check_blend_arg(b, n_frames, n_plain);
    if (rc != AID_OK) return rc;
    if (!dtype_ok(dtype)) return AID_ERR_DTYPE;
    if (k_fs < 8 || vt_fs < 8 || k_fs % 8 || vt_fs % 8) return AID_ERR_SHAPE;
    if (b->q8 && (vt_ld < 8 || vt_ld % 8 || vt_fs % vt_ld || vt_cols < 1 || vt_cols > vt_ld)) return AID_ERR_SHAPE;
    if (!aligned16(k2) || !aligned16(vt2)) return AID_ERR_SHAPE;
    return check_blend_shape(*b);
}

static int mix_kv_stores_impl(const aid::MixStoresArgs& ms, void* stream) {
    hipError_t e;
    {
        // traffic: block row *step of every store read once, one mixed row written per AID frame
        const double es = ms.dtype == AID_DTYPE_F32 ? 4.0 : 2.0, elems = (double)(ms.k_fs + ms.vt_fs);
        const double stored = ms.q8 ? (double)(ms.k_fs + (ms.k_fs + 31) / 32 + ms.vt_fs + (ms.vt_fs + 31) / 32) : es * elems;
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_mix_kv_stores<%s,m%d,%s>", dtype_name(ms.dtype), ms.n_corners, ms.q8 ? "q8" : "native");
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 2.0 * ms.n_corners * ms.n_mix * elems,
                     ms.n_corners * stored + es * ms.n_mix * elems);
        e = aid::mix_kv_stores_launch(ms, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_mix_kv_stores");
}

int aid_mix_kv_stores(const AidKeyframeBlend* b, void* k2, void* vt2, int32_t n_frames, int32_t n_plain, int64_t k_fs, int64_t vt_fs,
                      int32_t vt_ld, int32_t vt_cols, int32_t dtype, void* stream) {
    const int rc = check_mix_stores(b, k2, vt2, n_frames, n_plain, k_fs, vt_fs, vt_ld, vt_cols, dtype);
    if (rc != AID_OK) return rc;
    aid::MixStoresArgs ms;
    ms.rows = b->rows; ms.step = b->step; ms.weights = b->weights; ms.k2 = k2; ms.vt2 = vt2;
    ms.n_corners = b->n_corners; ms.n_steps = b->n_steps; ms.q8 = b->q8; ms.n_mix = n_frames - n_plain;
    ms.k_fs = k_fs; ms.vt_fs = vt_fs; ms.vt_ld = vt_ld; ms.vt_cols = vt_cols; ms.dtype = dtype;
    return mix_kv_stores_impl(ms, stream);
}

// the composition over aid_attn_fwd (aid_hip.h); `a` and `c` are checked, tab = the pair table's memory
// mix_src (INNER only): the corners are key-frame stores — the mix reads them instead of rows c.rows of a.k / a.vt
static int attn_corners_impl(const AidAttnArgs& a, const AidCorners& c, float* tab, void* stream,
                             const aid::MixStoresArgs* mix_src = nullptr) {
    const int n = a.n_frames, n_mix = a.n_frames - a.n_plain, M = c.n_corners;
    hipError_t e;
    {
        ProfScope ps(static_cast<hipStream_t>(stream), "aid_corner_pairs", 0.0, 4.0 * n * (M + 1.0 + 2.0 * ((M + 1) / 2)));
        e = aid::corner_pairs_launch(c.weights, tab, n, n_mix, M, static_cast<hipStream_t>(stream));
    }
    if (e != hipSuccess) return fail_hip(e, "aid_attn_corners_fwd");
    AidAttnArgs at = corner_pass0(a, c, tab);
    if (a.mode == AID_MODE_INNER) {             // every AID frame reads its mixed row (coefficient 0.5), the riders their own keys
        const int rc = mix_src ? mix_kv_stores_impl(*mix_src, stream)
                               : mix_kv_impl(a.k, a.vt, const_cast<void*>(a.k2), const_cast<void*>(a.vt2), c.rows, c.weights, n, a.n_plain,
                                             M, a.k_fs, a.vt_fs, a.dtype, stream);
        if (rc != AID_OK) return rc;
        return aid_attn_fwd(&at, stream);
    }
    int rc = aid_attn_fwd(&at, stream);         // OUTER pass 0: every frame, the riders with it
    for (int p = 1; p < (M + 1) / 2 && rc == AID_OK && n_mix > 0; ++p) {        // pass p: the AID frames, accumulating
        at.n_frames = n_mix;
        at.n_plain = 0;
        at.coef = tab + (size_t)(1 + 2 * p) * n;
        at.frame_scale = tab + (size_t)(2 + 2 * p) * n;
        at.begin = c.rows[2 * p];
        at.end = 2 * p + 1 < M ? c.rows[2 * p + 1] : c.rows[2 * p];
        at.accumulate = 1;
        rc = aid_attn_fwd(&at, stream);
    }
    return rc;
}

int aid_attn_corners_fwd(const AidAttnArgs* args, const AidCorners* corners, void* stream) {
    if (!args || !corners) return AID_ERR_ARG;
    const AidAttnArgs& a = *args;
    if (a.mode != AID_MODE_INNER && a.mode != AID_MODE_OUTER) return AID_ERR_ARG;
    int rc = check_corners(*corners, a.n_frames, a.n_kv, a.n_plain, true);
    if (rc != AID_OK) return rc;
    float* tab = static_cast<float*>(corners->scratch);
    const AidAttnArgs at = corner_pass0(a, *corners, tab);
    rc = check_attn(at);
    if (rc != AID_OK) return rc;
    if (a.mode == AID_MODE_INNER) {
        rc = check_mix(a.k, a.vt, a.k2, a.vt2, corners->rows, corners->weights, a.n_frames, a.n_plain, corners->n_corners, a.k_fs, a.vt_fs,
                       a.dtype);
        if (rc != AID_OK) return rc;
    }
    return attn_corners_impl(a, *corners, tab, stream);
}

size_t aid_processor_workspace_bytes(const AidProcessorArgs* args) {
    if (!args || check_processor(*args) != AID_OK) return 0;
    return carve(*args).total;
}

// The AidProcessorArgs a corner-weighted processor call is checked and carved with: coef / begin / end are not the caller's to give,
// so the weights (a non-NULL device pointer; the pair table replaces it before any kernel reads a coefficient) and the first corner
// stand in.  `extras`: image segments or a store came with the call.
static int corners_processor_args(const AidProcessorArgs& a, const AidCorners& c, bool extras, AidProcessorArgs* out) {
    if (a.mode != AID_MODE_INNER && a.mode != AID_MODE_OUTER) return AID_ERR_ARG;
    if (a.ip || extras) return AID_ERR_ARG;
    const int rc = check_corners(c, a.n_frames, a.ctx ? a.n_ctx : a.n_frames, a.n_plain, false);
    if (rc != AID_OK) return rc;
    *out = a;
    out->coef = c.weights;
    out->begin = out->end = c.rows[0];
    return AID_OK;
}

int aid_endpoint_rows(const AidEndpointRows* args, void* stream) {
    if (!args) return AID_ERR_ARG;
    const AidEndpointRows& a = *args;
    if (!a.k || !a.vt || !a.k_store || !a.vt_store || !a.step || !aligned4(a.step)) return AID_ERR_ARG;
    if (a.row_begin < 0 || a.row_end < 0 || a.n_steps < 1) return AID_ERR_ARG;
    if (a.direction != AID_EP_PUT && a.direction != AID_EP_GET) return AID_ERR_ARG;
    if (!dtype_ok(a.dtype)) return AID_ERR_DTYPE;
    if (a.k_fs < 8 || a.vt_fs < 8 || a.k_fs % 8 || a.vt_fs % 8) return AID_ERR_SHAPE;
    if (!aligned16(a.k) || !aligned16(a.vt) || !aligned16(a.k_store) || !aligned16(a.vt_store)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        // traffic: the four blocks read once and written once
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_endpoint_rows<%s,%s>", dtype_name(a.dtype), a.direction == AID_EP_PUT ? "put" : "get");
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 0.0, (a.dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * 4.0 * (double)(a.k_fs + a.vt_fs));
        e = aid::endpoint_rows_launch(a, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_endpoint_rows");
}

int aid_keyframe_rows(const AidKeyframeRows* args, void* stream) {
    if (!args) return AID_ERR_ARG;
    const AidKeyframeRows& a = *args;
    if (!a.k || !a.vt || !a.rows || !a.step || !aligned4(a.step)) return AID_ERR_ARG;
    if (a.n_rows < 1 || a.n_rows > AID_KF_MAX_ROWS || a.n_steps < 1) return AID_ERR_ARG;
    for (int i = 0; i < a.n_rows; ++i)
        if (!a.rows[i].k_store || !a.rows[i].vt_store || a.rows[i].row < 0) return AID_ERR_ARG;
    if (a.direction != AID_KF_PUT && a.direction != AID_KF_GET) return AID_ERR_ARG;
    if (!dtype_ok(a.dtype)) return AID_ERR_DTYPE;
    if (a.k_fs < 8 || a.vt_fs < 8 || a.k_fs % 8 || a.vt_fs % 8) return AID_ERR_SHAPE;
    if (!aligned16(a.k) || !aligned16(a.vt)) return AID_ERR_SHAPE;
    for (int i = 0; i < a.n_rows; ++i)
        if (!aligned16(a.rows[i].k_store) || !aligned16(a.rows[i].vt_store)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        // traffic: the two blocks of every entry read once and written once
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_keyframe_rows<%s,%s>", dtype_name(a.dtype), a.direction == AID_KF_PUT ? "put" : "get");
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 0.0,
                     (a.dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * 2.0 * a.n_rows * (double)(a.k_fs + a.vt_fs));
        e = aid::keyframe_rows_launch(a, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_keyframe_rows");
}

size_t aid_q8_block_bytes(int64_t n_elements) {
    if (n_elements < 8 || n_elements % 8) return 0;
    return (size_t)((n_elements + (n_elements + 31) / 32 + 15) / 16 * 16);
}

int aid_keyframe_rows_q8(const AidKeyframeRowsQ8* args, void* stream) {
    if (!args) return AID_ERR_ARG;
    const AidKeyframeRowsQ8& a = *args;
    if (!a.k || !a.vt || !a.rows || !a.step || !aligned4(a.step)) return AID_ERR_ARG;
    if (a.n_rows < 1 || a.n_rows > AID_KF_MAX_ROWS || a.n_steps < 1) return AID_ERR_ARG;
    for (int i = 0; i < a.n_rows; ++i)
        if (!a.rows[i].k_store || !a.rows[i].vt_store || a.rows[i].row < 0) return AID_ERR_ARG;
    if (a.direction != AID_KF_PUT && a.direction != AID_KF_GET) return AID_ERR_ARG;
    if (!dtype_ok(a.dtype)) return AID_ERR_DTYPE;
    if (a.k_fs < 8 || a.vt_fs < 8 || a.k_fs % 8 || a.vt_fs % 8) return AID_ERR_SHAPE;
    if (a.vt_ld < 8 || a.vt_ld % 8 || a.vt_fs % a.vt_ld || a.vt_cols < 1 || a.vt_cols > a.vt_ld) return AID_ERR_SHAPE;
    if (!aligned16(a.k) || !aligned16(a.vt)) return AID_ERR_SHAPE;
    for (int i = 0; i < a.n_rows; ++i)
        if (!aligned16(a.rows[i].k_store) || !aligned16(a.rows[i].vt_store)) return AID_ERR_SHAPE;
    hipError_t e;
    {
        // traffic: the two blocks of every entry on the call side, their int8 and exponent bytes on the store side
        char nm[64];
        snprintf(nm, sizeof(nm), "aid_keyframe_rows_q8<%s,%s>", dtype_name(a.dtype), a.direction == AID_KF_PUT ? "put" : "get");
        const double stored = (double)(a.k_fs + (a.k_fs + 31) / 32 + a.vt_fs + (a.vt_fs + 31) / 32);
        ProfScope ps(static_cast<hipStream_t>(stream), nm, 0.0,
                     a.n_rows * ((a.dtype == AID_DTYPE_F32 ? 4.0 : 2.0) * (double)(a.k_fs + a.vt_fs) + stored));
        e = aid::keyframe_rows_q8_launch(a, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? AID_OK : fail_hip(e, "aid_keyframe_rows_q8");
}

// end-point store beside a processor call (aid_hip.h): self-attention AID calls only
static int check_endpoint_store(const AidProcessorArgs& a, const AidEndpointStore& ep) {
    if (ep.mode != AID_EP_RECORD && ep.mode != AID_EP_REPLAY) return AID_ERR_ARG;
    if (a.ctx || a.mode == AID_MODE_PLAIN || a.ip) return AID_ERR_ARG;
    if (!ep.k_store || !ep.vt_store || !ep.step || !aligned4(ep.step) || ep.n_steps < 1) return AID_ERR_ARG;
    if (!aligned16(ep.k_store) || !aligned16(ep.vt_store)) return AID_ERR_SHAPE;
    return AID_OK;
}

// key-frame stores beside a processor call (aid_hip.h): RECORD on a PLAIN self-attention call, REPLAY on an AID one
static int check_keyframe_call(const AidProcessorArgs& a, const AidKeyframeCall& kf) {
    if (kf.mode != AID_KF_RECORD && kf.mode != AID_KF_REPLAY) return AID_ERR_ARG;
    if (a.ctx || a.ip) return AID_ERR_ARG;
    if ((kf.mode == AID_KF_RECORD) != (a.mode == AID_MODE_PLAIN)) return AID_ERR_ARG;
    if (!kf.rows || !kf.step || !aligned4(kf.step) || kf.n_steps < 1) return AID_ERR_ARG;
    if (kf.mode == AID_KF_REPLAY ? kf.n_rows != 2 : (kf.n_rows < 1 || kf.n_rows > AID_KF_MAX_ROWS)) return AID_ERR_ARG;
    for (int i = 0; i < kf.n_rows; ++i) {
        if (!kf.rows[i].k_store || !kf.rows[i].vt_store) return AID_ERR_ARG;
        if (kf.mode == AID_KF_RECORD) {
            if (kf.rows[i].row < 0 || kf.rows[i].row >= a.n_frames) return AID_ERR_ARG;
            for (int j = 0; j < i; ++j)
                if (kf.rows[j].row == kf.rows[i].row) return AID_ERR_ARG;
        }
    }
    for (int i = 0; i < kf.n_rows; ++i)
        if (!aligned16(kf.rows[i].k_store) || !aligned16(kf.rows[i].vt_store)) return AID_ERR_SHAPE;
    return AID_OK;
}

static int processor_impl(const AidProcessorArgs* args, const AidIpSegment* ip_segs, int32_t n_ip_segs, const AidEndpointStore* ep,
                          const AidKeyframeCall* kf, void* stream, bool kf_q8 = false, const AidCorners* cn = nullptr,
                          const AidKeyframeBlend* kb = nullptr);

size_t aid_processor_ep_workspace_bytes(const AidProcessorArgs* args, const AidEndpointStore* ep) {
    if (!args) return 0;
    if (!ep) return aid_processor_workspace_bytes(args);
    AidProcessorArgs a = *args;
    if (ep->mode == AID_EP_REPLAY) a.begin = a.end = 0;           // not read in replay
    if (check_processor(a) != AID_OK || check_endpoint_store(a, *ep) != AID_OK) return 0;
    return carve(a, ep->mode == AID_EP_REPLAY ? 2 : 0).total;
}

size_t aid_processor_kf_workspace_bytes(const AidProcessorArgs* args, const AidKeyframeCall* kf) {
    if (!args) return 0;
    if (!kf) return aid_processor_workspace_bytes(args);
    AidProcessorArgs a = *args;
    if (kf->mode == AID_KF_REPLAY) a.begin = a.end = 0;           // not read in replay
    if (check_processor(a) != AID_OK || check_keyframe_call(a, *kf) != AID_OK) return 0;
    return carve(a, kf->mode == AID_KF_REPLAY ? 2 : 0).total;
}

int aid_processor_fwd(const AidProcessorArgs* args, void* stream) { return processor_impl(args, nullptr, 0, nullptr, nullptr, stream); }

int aid_processor_ip_fwd(const AidProcessorArgs* args, const AidIpSegment* ip_segs, int32_t n_ip_segs, void* stream) {
    return processor_impl(args, ip_segs, n_ip_segs, nullptr, nullptr, stream);
}

int aid_processor_ep_fwd(const AidProcessorArgs* args, const AidEndpointStore* ep, void* stream) {
    return processor_impl(args, nullptr, 0, ep, nullptr, stream);
}

int aid_processor_kf_fwd(const AidProcessorArgs* args, const AidKeyframeCall* kf, void* stream) {
    return processor_impl(args, nullptr, 0, nullptr, kf, stream);
}

// the q8 stores change the copy launch alone: the checks and the workspace are aid_processor_kf_fwd's
size_t aid_processor_kf_q8_workspace_bytes(const AidProcessorArgs* args, const AidKeyframeCall* kf) {
    return aid_processor_kf_workspace_bytes(args, kf);
}

int aid_processor_kf_q8_fwd(const AidProcessorArgs* args, const AidKeyframeCall* kf, void* stream) {
    return processor_impl(args, nullptr, 0, nullptr, kf, stream, true);
}

size_t aid_processor_corners_workspace_bytes(const AidProcessorArgs* args, const AidCorners* corners) {
    if (!args) return 0;
    if (!corners) return aid_processor_workspace_bytes(args);
    AidProcessorArgs a;
    if (corners_processor_args(*args, *corners, false, &a) != AID_OK || check_processor(a) != AID_OK) return 0;
    return carve(a, 0, corners->n_corners).total;
}

int aid_processor_corners_fwd(const AidProcessorArgs* args, const AidCorners* corners, void* stream) {
    return processor_impl(args, nullptr, 0, nullptr, nullptr, stream, false, corners);
}

// The AidProcessorArgs a key-frame blend call is checked and carved with: a self-attention AID call over the local frames; as for a
// corner call the weights stand in for coef, and no end point is a row of the call (begin = end = 0).  Everything but the alignment
// rules of the AidKeyframeBlend (check_blend_shape, after check_processor: ARG, DTYPE, SHAPE in that order).
static int blend_processor_args(const AidProcessorArgs& a, const AidKeyframeBlend& b, AidProcessorArgs* out) {
    if (a.ctx || a.ip || (a.mode != AID_MODE_INNER && a.mode != AID_MODE_OUTER)) return AID_ERR_ARG;
    const int rc = check_blend_arg(&b, a.n_frames, a.n_plain);
    if (rc != AID_OK) return rc;
    *out = a;
    out->coef = b.weights;
    out->begin = out->end = 0;
    return AID_OK;
}

size_t aid_processor_kf_blend_workspace_bytes(const AidProcessorArgs* args, const AidKeyframeBlend* b) {
    if (!args) return 0;
    if (!b) return aid_processor_workspace_bytes(args);
    AidProcessorArgs a;
    if (blend_processor_args(*args, *b, &a) != AID_OK || check_processor(a) != AID_OK || check_blend_shape(*b) != AID_OK) return 0;
    return carve(a, a.mode == AID_MODE_OUTER ? b->n_corners : 0, b->n_corners).total;
}

int aid_processor_kf_blend_fwd(const AidProcessorArgs* args, const AidKeyframeBlend* b, void* stream) {
    return processor_impl(args, nullptr, 0, nullptr, nullptr, stream, false, nullptr, b);
}

// ``ep`` / ``kf`` (at most one of them): which copy launch stands behind the projections — a pair store's aid_endpoint_rows, the
// key-frame stores' aid_keyframe_rows or, with ``kf_q8``, aid_keyframe_rows_q8 on 8-bit block stores.  All replays are the same call:
// two rows more of k / V^T, filled by that launch.
// ``cn``: a corner-weighted call (aid_processor_corners_fwd) — step 2 is the composition among the corners, nothing else differs.
// ``kb`` (alone): that composition among recorded key frames (aid_processor_kf_blend_fwd) — OUTER: a replay with n_corners rows behind
// the local ones as the corners; INNER: no extra rows, the mix reads the stores.
static int processor_impl(const AidProcessorArgs* args, const AidIpSegment* ip_segs, int32_t n_ip_segs, const AidEndpointStore* ep,
                          const AidKeyframeCall* kf, void* stream, bool kf_q8, const AidCorners* cn, const AidKeyframeBlend* kb) {
    if (!args) return AID_ERR_ARG;
    AidProcessorArgs a_local;
    const bool replay = (ep && ep->mode == AID_EP_REPLAY) || (kf && kf->mode == AID_KF_REPLAY);
    if (replay) {                                         // the end points are rows n_frames / n_frames + 1 of k / V^T (filled from the
        a_local = *args;                                  // store below); args->begin / args->end are not read
        a_local.begin = a_local.end = 0;
    }
    if (cn) {                                             // args->coef / begin / end are not read: the pair table stands in for them
        const int rcc = corners_processor_args(*args, *cn, ip_segs != nullptr || n_ip_segs != 0 || ep || kf, &a_local);
        if (rcc != AID_OK) return rcc;
    }
    if (kb) {                                             // args->coef / begin / end are not read here either
        const int rcb = blend_processor_args(*args, *kb, &a_local);
        if (rcb != AID_OK) return rcb;
    }
    const AidProcessorArgs& a = (replay || cn || kb) ? a_local : *args;
    int rc = check_processor(a);
    if (rc != AID_OK) return rc;
    if (kb) {
        rc = check_blend_shape(*kb);
        if (rc != AID_OK) return rc;
    }
    if (ep) {
        rc = check_endpoint_store(a, *ep);
        if (rc != AID_OK) return rc;
    }
    if (kf) {
        rc = check_keyframe_call(a, *kf);
        if (rc != AID_OK) return rc;
    }
    if (n_ip_segs < 0 || (n_ip_segs == 0 && ip_segs)) return AID_ERR_ARG;
    if (n_ip_segs > 0) {                               // image segments: a cross-attention PLAIN call without the ip_* branch, 16-bit
        if (!a.ctx || a.mode != AID_MODE_PLAIN || a.ip) return AID_ERR_ARG;
        if (!dtype16(a.dtype)) return AID_ERR_DTYPE;
        rc = check_ip_segments(ip_segs, n_ip_segs, a.n_frames);
        if (rc != AID_OK) return rc;
    }
    const int kv_extra = replay ? 2 : (kb && a.mode == AID_MODE_OUTER) ? kb->n_corners : 0;
    const Carve cv = carve(a, kv_extra, cn ? cn->n_corners : kb ? kb->n_corners : 0);
    if (!a.workspace || a.workspace_bytes < cv.total || !aligned16(a.workspace)) return AID_ERR_WORKSPACE;
    char* ws = static_cast<char*>(a.workspace);
    void* q = ws + cv.q;
    const bool cached = a.k_cached != nullptr;           // step-invariant text keys / values: projected once by the caller
    const void* k = cached ? a.k_cached : ws + cv.k;
    const void* vt = cached ? a.vt_cached : ws + cv.vt;
    void* o = ws + cv.o;
    const bool cross = a.ctx != nullptr;
    const void* xin = a.x;
    const bool folded = a.ln_eps > 0.f && a.ln_wq != nullptr;
    float* stats = reinterpret_cast<float*>(ws + cv.xn);
    if (folded) {                              // 0. the block's norm1 / norm2, folded: only the row statistics are computed
        rc = aid_ln_stats(a.x, stats, (int64_t)a.n_frames * a.s, a.c, a.ln_eps, a.dtype, stream);
        if (rc != AID_OK) return rc;
    } else if (a.ln_eps > 0.f) {               // 0. ... or as its own pass
        void* xn = ws + cv.xn;
        rc = aid_layernorm(a.x, a.ln_gamma, a.ln_beta, xn, (int64_t)a.n_frames * a.s, a.c, a.ln_eps, a.dtype, stream);
        if (rc != AID_OK) return rc;
        xin = xn;
    }
    const void* e = cross ? a.ctx : xin;
    const int nctx = cross ? a.n_ctx : a.n_frames;
    const int l = cross ? a.l : a.s;
    const int cc = cross ? a.cc : a.c;
    const int d = a.c / a.heads;
    const size_t es = a.dtype == AID_DTYPE_F32 ? 4 : 2;

    // 0b. LoRA (ABI v9): U = input A_pack^T of x (q [, k, v]) and of ctx (k, v) in one grouped launch; the projections below add
    //     U B_pack^T to their accumulators (AidGemmProblem.lr_*)
    char* ux = ws + cv.ux;
    char* uctx = ws + cv.uctx;
    if (cv.rx || cv.rctx) {
        AidGemmProblem pd[2];
        memset(pd, 0, sizeof(pd));
        int nd = 0;
        if (cv.rx) {
            pd[nd].a = xin; pd[nd].b = a.lora_down_x; pd[nd].c = ux;
            pd[nd].m = a.n_frames * a.s; pd[nd].n = cv.rx; pd[nd].k = a.c;
            pd[nd].lda = a.c; pd[nd].ldb = a.c; pd[nd].ldc = cv.rx; pd[nd].batch = 1;
            ++nd;
        }
        if (cv.rctx) {
            pd[nd].a = a.ctx; pd[nd].b = a.lora_down_ctx; pd[nd].c = uctx;
            pd[nd].m = a.n_ctx * a.l; pd[nd].n = cv.rctx; pd[nd].k = a.cc;
            pd[nd].lda = a.cc; pd[nd].ldb = a.cc; pd[nd].ldc = cv.rctx; pd[nd].batch = 1;
            ++nd;
        }
        pd[0].cu_share = a.cu_share;
        for (int i = 0; i < nd; ++i) pd[i].f32_split = a.f32_split;
        rc = aid_gemm_nt(pd, nd, a.dtype, stream);
        if (rc != AID_OK) return rc;
    }

    // 1. q, k and V^T projections in one grouped launch
    AidGemmProblem pr[5];
    memset(pr, 0, sizeof(pr));
    pr[0].a = xin;  pr[0].b = a.wq; pr[0].c = q;
    pr[0].m = a.n_frames * a.s; pr[0].n = a.c; pr[0].k = a.c;
    pr[0].lda = a.c; pr[0].ldb = a.c; pr[0].ldc = a.c; pr[0].batch = 1;
    pr[0].scale = 1.4426950408889634f / sqrtf((float)d);      // softmax_scale * log2(e) folded into q before its rounding
    pr[0].cu_share = a.cu_share;
    pr[1].a = e;    pr[1].b = a.wk; pr[1].c = ws + cv.k;
    pr[1].m = nctx * l; pr[1].n = a.c; pr[1].k = cc;
    pr[1].lda = cc; pr[1].ldb = cc; pr[1].ldc = a.c; pr[1].batch = 1;
    pr[2].a = a.wv; pr[2].b = e;    pr[2].c = ws + cv.vt;    // V^T[b] = Wv * E_b^T  -> [c, l]
    pr[2].m = a.c; pr[2].n = l; pr[2].k = cc;
    pr[2].lda = cc; pr[2].ldb = cc; pr[2].ldc = cv.lp; pr[2].batch = nctx;
    pr[2].stride_a = 0; pr[2].stride_b = (int64_t)l * cc; pr[2].stride_c = (int64_t)a.c * cv.lp;
    if (!cross && l % 8 == 0) {
        // self-attention: the FLAT value projection x Wv^T with the transposed epilogue (AidGemmProblem.trans_rows) — the same
        // V^T, but its tiles count like the q / k projections' (the 288-row engine then runs all three in whole CU rounds)
        pr[2].a = e;    pr[2].b = a.wv;
        pr[2].m = nctx * l; pr[2].n = a.c; pr[2].k = cc;
        pr[2].lda = cc; pr[2].ldb = cc; pr[2].ldc = cv.lp; pr[2].batch = 1;
        pr[2].stride_a = 0; pr[2].stride_b = 0; pr[2].stride_c = (int64_t)a.c * cv.lp;
        pr[2].trans_rows = l;
    }
    if (folded) {                                             // x W'^T with the LayerNorm applied in the epilogue
        pr[0].b = a.ln_wq;
        pr[0].ln_stats = stats; pr[0].ln_colsum = a.ln_const; pr[0].ln_shift = a.ln_const + a.c; pr[0].ln_side = 1;
        if (!cross) {
            pr[1].b = a.ln_wk;
            pr[1].ln_stats = stats; pr[1].ln_colsum = a.ln_const + 2 * a.c; pr[1].ln_shift = a.ln_const + 3 * a.c;
            pr[1].ln_side = 1;
            pr[2].ln_stats = stats; pr[2].ln_colsum = a.ln_const + 4 * a.c; pr[2].ln_shift = a.ln_const + 5 * a.c;
            if (pr[2].trans_rows) { pr[2].b = a.ln_wv; pr[2].ln_side = 1; }
            else                  { pr[2].a = a.ln_wv; pr[2].ln_side = 2; pr[2].stride_stats = l; }
        }
    }
    if (a.lora_r_q) {
        pr[0].lr_a = ux; pr[0].lr_lda = cv.rx;
        pr[0].lr_b = a.lora_up_q; pr[0].lr_ldb = a.lora_r_q; pr[0].lr_k = a.lora_r_q;
        pr[0].lr_row_scale = a.lora_gain_q; pr[0].lr_scale_side = 2;
    }
    {
        char* ue = cross ? uctx : ux;                         // U of the keys' / values' input, its columns, and where k / v start
        const int re = cross ? cv.rctx : cv.rx;
        const size_t ok = cross ? 0 : (size_t)a.lora_r_q, ov = ok + a.lora_r_k;
        if (a.lora_r_k) {
            pr[1].lr_a = ue + ok * es; pr[1].lr_lda = re;
            pr[1].lr_b = a.lora_up_k; pr[1].lr_ldb = a.lora_r_k; pr[1].lr_k = a.lora_r_k;
            pr[1].lr_row_scale = a.lora_gain_k; pr[1].lr_scale_side = 2;
        }
        if (a.lora_r_v) {
            pr[2].lr_k = a.lora_r_v;
            pr[2].lr_row_scale = a.lora_gain_v;                 // DoRA: indexed by the weight's rows, n in the flat form, m in the batched
            pr[2].lr_scale_side = pr[2].trans_rows ? 2 : 1;
            if (pr[2].trans_rows) {                           // flat x Wv^T: LA = U_v (rows like x), LB = B_v
                pr[2].lr_a = ue + ov * es; pr[2].lr_lda = re;
                pr[2].lr_b = a.lora_up_v; pr[2].lr_ldb = a.lora_r_v;
            } else {                                          // V^T[f] = Wv E_f^T: LA = B_v (shared), LB = U_v[f]
                pr[2].lr_a = a.lora_up_v; pr[2].lr_lda = a.lora_r_v;
                pr[2].lr_b = ue + ov * es; pr[2].lr_ldb = re; pr[2].lr_stride_b = (int64_t)l * re;
            }
        }
    }
    int npr = 3;
    void* kip = ws + cv.kip;
    void* vtip = ws + cv.vtip;
    if (a.ip) {                                               // K_ip = to_k_ip(ip rows), V_ip^T = Wv_ip * ip_row^T
        pr[3].a = a.ip; pr[3].b = a.wk_ip; pr[3].c = kip;
        pr[3].m = a.t_ip; pr[3].n = a.c; pr[3].k = a.cc;
        pr[3].lda = a.cc; pr[3].ldb = a.cc; pr[3].ldc = a.c; pr[3].batch = a.n_ip;
        pr[3].stride_a = a.ip_stride; pr[3].stride_b = 0; pr[3].stride_c = (int64_t)a.t_ip * a.c;
        pr[4].a = a.wv_ip; pr[4].b = a.ip; pr[4].c = vtip;
        pr[4].m = a.c; pr[4].n = a.t_ip; pr[4].k = a.cc;
        pr[4].lda = a.cc; pr[4].ldb = a.cc; pr[4].ldc = cv.tp; pr[4].batch = a.n_ip;
        pr[4].stride_a = 0; pr[4].stride_b = a.ip_stride; pr[4].stride_c = (int64_t)a.c * cv.tp;
        npr = 5;
    }
    if (cached) {                                             // the query projection (and the image keys / values) only
        for (int i = 3; i < npr; ++i) pr[i - 2] = pr[i];
        npr -= 2;
        pr[0].cu_share = a.cu_share;
    }
    for (int i = 0; i < npr; ++i) pr[i].f32_split = a.f32_split;
    rc = aid_gemm_nt(pr, npr, a.dtype, stream);
    if (rc != AID_OK) return rc;

    // 1b. end-point store: RECORD keeps the end-point rows of this step's k / V^T, REPLAY puts the recorded rows behind the local ones
    const int kv_rows = nctx + kv_extra;
    const int begin = replay ? nctx : a.begin, end = replay ? nctx + 1 : a.end;
    if (ep) {
        AidEndpointRows er;
        memset(&er, 0, sizeof(er));
        er.k = ws + cv.k; er.vt = ws + cv.vt; er.k_store = ep->k_store; er.vt_store = ep->vt_store;
        er.step = ep->step; er.n_steps = ep->n_steps;
        er.k_fs = (int64_t)l * a.c; er.vt_fs = (int64_t)a.c * cv.lp;
        er.row_begin = begin; er.row_end = end;
        er.direction = replay ? AID_EP_GET : AID_EP_PUT;
        er.dtype = a.dtype;
        rc = aid_endpoint_rows(&er, stream);
        if (rc != AID_OK) return rc;
    }
    if (kf) {                                                 // key-frame stores: the same two rows (REPLAY) / the key frames' rows (RECORD)
        AidKeyframeRow two[2];
        AidKeyframeRows kr;
        memset(&kr, 0, sizeof(kr));
        kr.k = ws + cv.k; kr.vt = ws + cv.vt; kr.rows = kf->rows; kr.n_rows = kf->n_rows;
        if (replay) {
            two[0] = kf->rows[0]; two[0].row = begin;
            two[1] = kf->rows[1]; two[1].row = end;
            kr.rows = two;
        }
        kr.step = kf->step; kr.n_steps = kf->n_steps;
        kr.k_fs = (int64_t)l * a.c; kr.vt_fs = (int64_t)a.c * cv.lp;
        kr.direction = replay ? AID_KF_GET : AID_KF_PUT;
        kr.dtype = a.dtype;
        if (kf_q8) {                                          // the same rows, (de)quantised in the lane; the keys are the stored columns
            AidKeyframeRowsQ8 kq;
            memset(&kq, 0, sizeof(kq));
            kq.k = kr.k; kq.vt = kr.vt; kq.rows = kr.rows; kq.step = kr.step;
            kq.k_fs = kr.k_fs; kq.vt_fs = kr.vt_fs; kq.vt_ld = cv.lp; kq.vt_cols = l;
            kq.n_rows = kr.n_rows; kq.n_steps = kr.n_steps; kq.direction = kr.direction; kq.dtype = kr.dtype;
            rc = aid_keyframe_rows_q8(&kq, stream);
        } else {
            rc = aid_keyframe_rows(&kr, stream);
        }
        if (rc != AID_OK) return rc;
    }
    int32_t blend_rows[AID_MAX_CORNERS] = {0, 0, 0, 0, 0, 0, 0, 0};      // the corners of a blend call as rows of k / V^T (INNER: none)
    if (kb && kv_extra) {                                     // OUTER blend: one GET of the M key frames' rows behind the local ones
        AidKeyframeRow rows[AID_KF_MAX_ROWS];
        for (int m = 0; m < kb->n_corners; ++m) {
            rows[m] = kb->rows[m];
            rows[m].row = blend_rows[m] = nctx + m;
        }
        AidKeyframeRowsQ8 kq;
        memset(&kq, 0, sizeof(kq));
        kq.k = ws + cv.k; kq.vt = ws + cv.vt; kq.rows = rows; kq.step = kb->step;
        kq.k_fs = (int64_t)l * a.c; kq.vt_fs = (int64_t)a.c * cv.lp; kq.vt_ld = cv.lp; kq.vt_cols = l;
        kq.n_rows = kb->n_corners; kq.n_steps = kb->n_steps; kq.direction = AID_KF_GET; kq.dtype = a.dtype;
        if (kb->q8) {
            rc = aid_keyframe_rows_q8(&kq, stream);
        } else {
            AidKeyframeRows kr;
            memset(&kr, 0, sizeof(kr));
            kr.k = kq.k; kr.vt = kq.vt; kr.rows = rows; kr.step = kq.step; kr.k_fs = kq.k_fs; kr.vt_fs = kq.vt_fs;
            kr.n_rows = kq.n_rows; kr.n_steps = kq.n_steps; kr.direction = AID_KF_GET; kr.dtype = a.dtype;
            rc = aid_keyframe_rows(&kr, stream);
        }
        if (rc != AID_OK) return rc;
    }

    // 2. interpolated attention core (INNER: interpolated K / V^T of the interior frames first)
    AidAttnArgs at;
    memset(&at, 0, sizeof(at));
    at.q = q; at.k = k; at.vt = vt; at.out = o;
    if (a.mode == AID_MODE_INNER) {
        // begin / end are rows of k / vt (context rows when ctx_map is given); the interpolated rows are per FRAME
        at.k2 = ws + cv.k2; at.vt2 = ws + cv.vt2;
        const int interior = a.n_frames - a.n_plain - 2;
        if (!cn && !kb) {                                     // (a corner / blend call mixes its own rows, below)
            rc = lerp_kv_impl(k, vt, ws + cv.k2, ws + cv.vt2, a.coef, a.n_frames, begin, end, (int64_t)l * a.c,
                              (int64_t)a.c * cv.lp, a.dtype, stream, interior > 0 ? interior : 0);
            if (rc != AID_OK) return rc;
        }
    }
    at.coef = a.coef; at.frame_scale = nullptr; at.kv_map = a.ctx_map;
    at.n_frames = a.n_frames; at.n_kv = kv_rows;
    at.s = a.s; at.l = l; at.heads = a.heads; at.d = d;
    at.ldq = a.c; at.ldk = a.c; at.ldvt = cv.lp; at.ldo = a.c;
    at.q_fs = (int64_t)a.s * a.c; at.k_fs = (int64_t)l * a.c; at.vt_fs = (int64_t)a.c * cv.lp; at.o_fs = (int64_t)a.s * a.c;
    at.bias = a.attn_bias; at.bias_fs = a.attn_bias_fs; at.bias_hs = a.attn_bias_hs; at.bias_rs = a.attn_bias_rs;
    at.mode = a.mode; at.fused = a.fused; at.begin = begin; at.end = end;
    at.accumulate = 0; at.dtype = a.dtype;
    at.softmax_scale = 1.0f / sqrtf((float)d);
    at.out_scale = 1.0f;
    at.n_plain = a.n_plain;
    at.q_prescaled = 1;
    at.seg_executed = a.seg_executed;
    at.f32_split = a.f32_attn_split;                          // (the image branch below copies it with the rest)
    if (kb) {
        AidCorners bc;
        memset(&bc, 0, sizeof(bc));
        bc.rows = blend_rows; bc.weights = kb->weights; bc.n_corners = kb->n_corners;
        aid::MixStoresArgs ms;
        ms.rows = kb->rows; ms.step = kb->step; ms.weights = kb->weights; ms.k2 = ws + cv.k2; ms.vt2 = ws + cv.vt2;
        ms.n_corners = kb->n_corners; ms.n_steps = kb->n_steps; ms.q8 = kb->q8; ms.n_mix = a.n_frames - a.n_plain;
        ms.k_fs = at.k_fs; ms.vt_fs = at.vt_fs; ms.vt_ld = cv.lp; ms.vt_cols = l; ms.dtype = a.dtype;
        rc = attn_corners_impl(at, bc, reinterpret_cast<float*>(ws + cv.ctab), stream, a.mode == AID_MODE_INNER ? &ms : nullptr);
    } else {
        rc = cn ? attn_corners_impl(at, *cn, reinterpret_cast<float*>(ws + cv.ctab), stream) : aid_attn_fwd(&at, stream);
    }
    if (rc != AID_OK) return rc;

    // 2b. IP-Adapter image branch: a second (short) attention launch that accumulates into o
    if (a.ip) {
        AidAttnArgs ai = at;
        ai.k = kip; ai.vt = vtip; ai.k2 = nullptr; ai.vt2 = nullptr;
        ai.kv_map = a.ip_map; ai.n_kv = a.n_ip; ai.l = a.t_ip;
        ai.bias = nullptr;
        ai.ldk = a.c; ai.ldvt = cv.tp;
        ai.k_fs = (int64_t)a.t_ip * a.c; ai.vt_fs = (int64_t)a.c * cv.tp;
        ai.accumulate = 1; ai.out_scale = a.ip_scale; ai.frame_scale = a.ip_frame_scale;
        ai.seg_executed = 0;
        if (a.ip_mode == AID_IP_SAME) {                   // same scheme as the text keys (OUTER), image end-point rows
            ai.begin = a.ip_begin; ai.end = a.ip_end;
        } else {                                          // every frame with its own image keys
            ai.mode = AID_MODE_PLAIN; ai.fused = 0; ai.coef = nullptr; ai.begin = 0; ai.end = 0; ai.n_plain = 0;
        }
        rc = aid_attn_fwd(&ai, stream);
        if (rc != AID_OK) return rc;
    }

    // 2c. image segments (several IP-Adapters / regional masks): all of them in one launch per AID_IP_MAX_SEGMENTS, into o
    for (int g0 = 0; g0 < n_ip_segs; g0 += AID_IP_MAX_SEGMENTS) {
        AidIpAttnArgs is;
        memset(&is, 0, sizeof(is));
        is.q = q; is.out = o;
        is.segments = ip_segs + g0;
        is.n_segments = n_ip_segs - g0 < AID_IP_MAX_SEGMENTS ? n_ip_segs - g0 : AID_IP_MAX_SEGMENTS;
        is.n_frames = a.n_frames; is.s = a.s; is.heads = a.heads; is.d = d;
        is.ldq = a.c; is.ldo = a.c;
        is.q_fs = (int64_t)a.s * a.c; is.o_fs = (int64_t)a.s * a.c;
        is.dtype = a.dtype;
        is.softmax_scale = 1.0f / sqrtf((float)d);
        is.q_prescaled = 1;
        rc = aid_ip_attn_fwd(&is, stream);
        if (rc != AID_OK) return rc;
    }

    // 3. out projection + bias (LoRA on to_out: U_o = o A_o^T first)
    AidGemmProblem po;
    memset(&po, 0, sizeof(po));
    po.a = o; po.b = a.wo; po.c = a.y; po.bias = a.bo; po.residual = a.residual;
    po.m = a.n_frames * a.s; po.n = a.c; po.k = a.c;
    po.lda = a.c; po.ldb = a.c; po.ldc = a.c; po.batch = 1;
    po.cu_share = a.cu_share;
    po.f32_split = a.f32_split;
    if (a.lora_r_o) {
        AidGemmProblem pd;
        memset(&pd, 0, sizeof(pd));
        pd.a = o; pd.b = a.lora_down_o; pd.c = ws + cv.uo;
        pd.m = a.n_frames * a.s; pd.n = a.lora_r_o; pd.k = a.c;
        pd.lda = a.c; pd.ldb = a.c; pd.ldc = a.lora_r_o; pd.batch = 1;
        pd.cu_share = a.cu_share;
        pd.f32_split = a.f32_split;
        rc = aid_gemm_nt(&pd, 1, a.dtype, stream);
        if (rc != AID_OK) return rc;
        po.lr_a = ws + cv.uo; po.lr_lda = a.lora_r_o;
        po.lr_b = a.lora_up_o; po.lr_ldb = a.lora_r_o; po.lr_k = a.lora_r_o;
        po.lr_row_scale = a.lora_gain_o; po.lr_scale_side = 2;
    }
    return aid_gemm_nt(&po, 1, a.dtype, stream);
}

}  // extern "C"
