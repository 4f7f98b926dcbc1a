/*
 * aid_hip.h — C ABI of libaid_hip.so: the MI355X (gfx950 / CDNA4) implementation of the
 * interpolated-attention hot path of QY-H00/attention-interpolation-diffusion.
 *
 * Plain pointers and sizes only: no torch / HIP types appear in any signature, so the
 * library can be bound from ctypes (what this repository's Python processors do), cffi,
 * pybind11 or any other FFI.  All pointers are DEVICE pointers unless stated otherwise;
 * `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 * Every entry point only enqueues work on `stream`: no allocation, no host
 * synchronisation, no hidden copies.  Return value: AID_OK (0) or a negative AID_ERR_*
 * code; aid_strerror() gives the text.  No C++ exception crosses this boundary.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   aid_processor_fwd      <- InterpolatedAttnProcessor family __call__ bodies:
 *                             OuterInterpolatedAttnProcessor   interpolation.py:573-679
 *                             InnerInterpolatedAttnProcessor   interpolation.py:707-804
 *                             de-activated fallback (AttnProcessor2_0)  interpolation.py:581-584
 *                             IP-Adapter variants (image branch = the ip_* fields):
 *                             OuterInterpolatedIPAttnProcessor  interpolation.py:240-387
 *                             InnerInterpolatedIPAttnProcessor  interpolation.py:417-545
 *                             ScaleControlIPAttnProcessor       interpolation.py:76-211
 *                             de-activated IP fallback (diffusers IPAdapterAttnProcessor2_0, called at
 *                             interpolation.py:248-251 / 425-428; semantics SURVEY.md App. A)
 *   aid_gemm_nt            <- attn.to_q / to_k / to_v / to_out[0]   interpolation.py:613,623-624,666
 *   aid_attn_fwd           <- end-point select / replicate / concat / get_attention_scores /
 *                             bmm / batch_to_head_dim / outer|inner lerp
 *                             interpolation.py:626-664 (outer), 760-790 (inner)
 */
#ifndef AID_HIP_H
#define AID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AID_ABI_VERSION 10

/* element types of activations / weights (accumulation is always fp32) */
#define AID_DTYPE_F16  0
#define AID_DTYPE_BF16 1
/* ABI v7: float32 tensors in and out, float32 arithmetic (v_mfma_f32_32x32x2_f32, the f32 vector rate) — the reference's own default
 * for SD1.x (gradio_src/app.py:62, 414) and its CPU path.  aid_gemm_nt, aid_attn_fwd, aid_lerp_kv and aid_processor_fwd take it
 * (probabilities are then not rounded before the PV product, like the reference's float32 get_attention_scores); the LayerNorm
 * entry points and the ln_* options of aid_processor_fwd are 16-bit only (AID_ERR_DTYPE); `residual` works with every dtype. */
#define AID_DTYPE_F32  2

/* image branch of the IP-Adapter processors (AidProcessorArgs.ip_mode) */
#define AID_IP_NONE       0
#define AID_IP_SAME       1
#define AID_IP_PLAIN      2

/* attention modes */
#define AID_MODE_PLAIN 0   /* softmax(Q K_i^T) V_i                       (AID de-activated)          */
#define AID_MODE_INNER 1   /* keys/values lerped between the end-point frames before attention     */
#define AID_MODE_OUTER 2   /* attention against each end-point frame, outputs lerped               */

/* error codes */
#define AID_OK             0
#define AID_ERR_ARG       -1   /* NULL pointer / negative size / inconsistent field              */
#define AID_ERR_DTYPE     -2   /* dtype not one of AID_DTYPE_*                                    */
#define AID_ERR_SHAPE     -3   /* unsupported head dim / alignment (see each function)            */
#define AID_ERR_WORKSPACE -4   /* workspace too small                                             */
#define AID_ERR_LAUNCH    -5   /* hipLaunchKernel failed (hipGetLastError text via aid_strerror)  */
#define AID_ERR_NO_DEVICE -6   /* no gfx950 device visible                                        */

/* ---------------------------------------------------------------------------------------
 * Grouped "NT" GEMM:   C[b] = A[b] * B[b]^T (+ bias)        for b in [0, batch)
 *   A [m, k] row-major (lda), B [n, k] row-major (ldb)  -> both operands K-contiguous,
 *   C [m, n] row-major (ldc).  bias (optional) is indexed by n and has the operand dtype.
 *   Up to AID_GEMM_MAX_PROBLEMS independent problems run in ONE launch (q, k and V^T
 *   projections of an attention layer).
 *   `residual` (optional, laid out like C incl. stride_c) is added AFTER the result was rounded to the
 *   operand dtype: C = round(round(scale * A B^T + bias) + residual) — bit for bit the reference's separate
 *   `hidden_states = attn_output + hidden_states` on the out-projection.
 *   Requirements: k % 8 == 0, lda % 8 == 0, ldb % 8 == 0, ldc % 4 == 0, ldc >= round_up(n, 4),
 *   all base pointers 16-byte aligned.  Columns [n, round_up(n,4)) of C are written with zeros.
 * ------------------------------------------------------------------------------------- */
#define AID_GEMM_MAX_PROBLEMS 6

typedef struct AidGemmProblem {
    const void* a;
    const void* b;
    void*       c;
    const void* bias;          /* NULL = none */
    int32_t     m, n, k;
    int32_t     lda, ldb, ldc; /* in elements */
    int32_t     batch;         /* >= 1 */
    float       scale;         /* C = scale * (A B^T) + bias; 0 means 1 (zero-initialised structs)  */
    int64_t     stride_a, stride_b, stride_c;   /* per-batch strides in elements (0 = shared) */
    const void* residual;      /* NULL = none; [m, ldc] per batch like C, operand dtype               */
    /* LayerNorm folded into the projection (ln_stats == NULL: none).  The ACTIVATION operand is un-normalised x, the     */
    /* WEIGHT operand is W' = W * gamma (aid_ln_fold), and the epilogue computes, before `scale` and `bias`,              */
    /*     LayerNorm(x) W^T = rstd * (x W'^T - mean * ln_colsum) + ln_shift                                               */
    /* ln_side 1: A is the activation (statistics row m, weight constants column n); 2: B is (statistics by n, constants  */
    /* by m — the V^T = Wv x^T problem).  ln_stats: fp32 [activation rows, 2] = (mean, rstd) from aid_ln_stats, batch b   */
    /* starts at row b * stride_stats; ln_colsum / ln_shift: fp32 [weight rows] from aid_ln_fold.                          */
    const float* ln_stats;
    const float* ln_colsum;
    const float* ln_shift;
    int32_t      ln_side;
    /* trans_rows > 0: C is written TRANSPOSED per frame of `trans_rows` rows: element (row m, column j) goes to          */
    /*     c + (m / trans_rows) * stride_c + j * ldc + m % trans_rows                                                     */
    /* i.e. V^T[frame][channel][key] from the flat value projection  E Wv^T  (a = E [frames * keys, k], b = Wv [n, k]),    */
    /* the layout the attention core reads.  Requirements: batch == 1, m % trans_rows == 0, trans_rows % 8 == 0,          */
    /* ldc >= trans_rows, ldc % 8 == 0, stride_c % 8 == 0, no bias, no residual, ln_side 1 if LayerNorm is folded.         */
    /* (Same numbers as the batched form  V^T[f] = Wv E_f^T; the library picks whichever its tile engines run faster.)    */
    int32_t      trans_rows;
    int64_t      stride_stats;
    /* ABI v7.  cu_share (read from problems[0]): n > 1 says that n independent launch streams of the CALLER run side by side (the   */
    /* conditional and the unconditional UNet call of a step on two streams), so this launch should plan with 1 / n of the CUs —    */
    /* a per-call hint (two host threads may pass different values); results never depend on it.  0 / 1: the whole device.          */
    int32_t      cu_share;
    /* float32 matmul precision (AID_DTYPE_F32 only; torch.set_float32_matmul_precision).  This is the field that was `reserved0`, which */
    /* callers left zero: layout and ABI version are unchanged.  0 (a zeroed struct): exact fp32 products on v_mfma_f32_32x32x2_f32.      */
    /* 1 ("high"): every operand element is taken as the sum of two bfloat16 numbers,                                                     */
    /*     Xh = bf16_rne(X),  Xl = bf16_rne(X - float(Xh))        (round-to-nearest-even both; the subtraction is exact in fp32)       */
    /*     C = epilogue( sum_k (Ah Bh + Al Bh + Ah Bl) )          (three v_mfma_f32_32x32x16_bf16 products, exact, fp32 accumulation)  */
    /* with the epilogue of the exact kernel: ~4e-6 rel-L2 of the fp64 product instead of ~3e-7, at 1.2 - 2.4 x the exact kernel's rate. */
    /* "May use": a launch runs split only if EVERY problem of the group asks for it and none carries ln_stats or a low-rank segment;  */
    /* every other group runs exact (never an error, nothing dropped).  An infinite or over-range element (|x| > 3.39e38) gives NaN    */
    /* where the exact kernel gives inf.  AID_ERR_ARG: a value outside {0, 1}; a non-zero value with a 16-bit dtype.                   */
    int32_t      f32_split;
    /* ABI v9 — low-rank second K segment (lr_k == 0: none): an unmerged LoRA adapter of the projection,                     */
    /*     C = epilogue( scale * (A B^T + LA LB^T) + bias ... )                                                               */
    /* LA = lr_a [m, lr_k] (row stride lr_lda), LB = lr_b [n, lr_k] (row stride lr_ldb), batch b at lr_a + b * lr_stride_a /   */
    /* lr_b + b * lr_stride_b (0 = shared).  The term accumulates in fp32 with the main product, before every epilogue step.   */
    /* Requirements: lr_k % 64 == 0, lr_k <= 512, lr_lda / lr_ldb % 8 == 0 and >= lr_k, lr_stride_* % 8 == 0, 16-byte bases;  */
    /* not with ln_stats (AID_ERR_ARG: the folded LayerNorm's correction would scale the term too).  trans_rows, bias,        */
    /* residual, batch > 1 and cu_share work as without it.  With trans_rows LA has the m = frames * rows layout of A (the     */
    /* flat value projection: LA = U_v, LB = B_v); the batched V^T[f] = Wv E_f^T form takes LA = B_v (stride 0), LB = U_v[f]. */
    const void*  lr_a;
    const void*  lr_b;
    int32_t      lr_k;
    int32_t      lr_lda;
    int32_t      lr_ldb;
    int32_t      lr_scale_side;  /* ABI v10: which dimension lr_row_scale is indexed by (below); ignored without it */
    int64_t      lr_stride_a;
    int64_t      lr_stride_b;
    /* ABI v10 — gain on the weight rows of a problem with a low-rank segment (NULL: none): a DoRA adapter,                      */
    /*     C = epilogue( scale * gain o (A B^T + LA LB^T) + bias ... )                                                           */
    /* The fp32 accumulator is multiplied by the fp32 gain after the low-rank segment and before every epilogue step (the scale,  */
    /* bias, rounding, residual and the transposed-per-frame store).  lr_scale_side 2: the weight operand is b, the gain is       */
    /* indexed by column n and has n entries; 1: the weight operand is a (the batched V^T[f] = Wv E_f^T form), the gain is        */
    /* indexed by row m and has m entries.  One gain for all batches (no stride).  With trans_rows the side is 2 (the gain is     */
    /* applied before the transposition).  AID_ERR_ARG: with lr_k == 0, a side other than 1 / 2, a base that is not 4-byte        */
    /* aligned; with ln_stats the segment itself is refused.  aid_dora_gain computes the gain of a DoRA layer.                    */
    const float* lr_row_scale;
} AidGemmProblem;

int aid_gemm_nt(const AidGemmProblem* problems /* host */, int n_problems, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * ABI v10.  Row gain of a DoRA adapter (PEFT's DoRA layers in eval mode; weights only, so once per adapter pack):
 *   gain[n] = magnitude[n] / || W[n, :] + (B_pack A_pack)[n, :] ||_2          (no epsilon, like PEFT)
 *   w [n_out, n_in] (row stride ldw) the base weight, a_pack [rank, n_in] the adapter's lora_A rows with its scaling folded
 *   in, b_pack [n_out, rank] its lora_B (both contiguous, zero-padded to `rank`: the operands of the low-rank segment),
 *   magnitude [n_out] — all in the storage dtype (f16 / bf16 / f32); gain [n_out] fp32.  The row W + B A is formed and squared
 *   in fp32 and never written.  With AidGemmProblem.lr_row_scale = gain the projection computes PEFT's DoRA forward
 *   gain o (x W^T + s B A x) + bias.
 * Requirements: n_in % 8 == 0, ldw % 8 == 0, ldw >= n_in, rank % 64 == 0, 64 <= rank <= 512, w / a_pack / b_pack / magnitude
 * 16-byte aligned (AID_ERR_SHAPE), gain 4-byte aligned.  Reads exactly the [n_out, n_in] / [rank, n_in] / [n_out, rank] / [n_out]
 * elements, writes exactly n_out floats.  One launch, no allocation, no synchronisation.
 * ------------------------------------------------------------------------------------- */
int aid_dora_gain(const void* w, const void* a_pack, const void* b_pack, const void* magnitude, float* gain, int32_t n_out,
                  int32_t n_in, int32_t ldw, int32_t rank, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Classifier-free guidance with the guidance rescale of arXiv 2305.08891 §3.4 — the combine the reference's loop runs between
 * its two UNet passes and scheduler.step (pipeline_interpolated_sd.py:92-108, 1892-1902) — in one launch.  Per sample i of n,
 * over the e elements of the sample, all arithmetic in fp32:
 *   c   = u + guidance_scale * (t - u)                        t = text[i], u = uncond[i]
 *   s_t = std(t), s_c = std(c)                                unbiased (e - 1), two-pass
 *   out = c * (guidance_rescale * s_t / s_c + (1 - guidance_rescale))          one rounding to the storage dtype
 * guidance_rescale 0 gives the plain combine c.  text / uncond / out [n, e] in the storage dtype (f16 / bf16 / f32), sample i
 * at base + i * stride ELEMENTS, the e elements of a sample contiguous: the two halves of a batched [2 n, e] UNet output are two
 * pointers into one tensor.  out may BE text or uncond (same base and stride); any other overlap of out with an input is refused.
 * One workgroup per sample; 16-byte loads and stores for every sample whose three bases are 16-byte aligned, scalar otherwise
 * and for the last e % 8 (f32: e % 4) elements.  s_c == 0 gives Inf / NaN, as the reference's division does.
 * AID_ERR_ARG: a NULL pointer, n < 0, a stride < e, guidance_rescale outside [0, 1], partial overlap of out with an input;
 * AID_ERR_SHAPE: e < 2, a pointer not aligned to the element size; AID_ERR_DTYPE; AID_ERR_NO_DEVICE.  n == 0 launches nothing.
 * Reads exactly the n * e elements of text and of uncond, writes exactly the n * e elements of out.  One launch, no allocation,
 * no synchronisation; capturable.
 * ------------------------------------------------------------------------------------- */
int aid_cfg_rescale(const void* text, const void* uncond, void* out, int32_t n, int64_t e, int64_t text_stride,
                    int64_t uncond_stride, int64_t out_stride, float guidance_scale, float guidance_rescale, int32_t dtype,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * LayerNorm over the last dimension: y[r, :] = (x[r, :] - mean_r) * rsqrt(var_r + eps) * gamma + beta
 * — the norm1 / norm2 in front of the attention call in diffusers' BasicTransformerBlock (the step
 * before the path).  fp32 statistics, one rounding; gamma / beta may be NULL.
 * Requirements: c % 8 == 0, 8 <= c <= 2048, x / y / gamma / beta 16-byte aligned, rows contiguous.
 * ------------------------------------------------------------------------------------- */
int aid_layernorm(const void* x, const void* gamma, const void* beta, void* y, int64_t rows, int32_t c,
                  float eps, int32_t dtype, void* stream);

/* The same LayerNorm FOLDED into the projections that consume it, so that LayerNorm(x) is never written or re-read:
 *   aid_ln_stats   stats[r] = (mean_r, rsqrt(var_r + eps)), fp32 [rows, 2] — one read of x, same arithmetic as aid_layernorm
 *   aid_ln_fold    once per (weight, gamma, beta): w_folded = w * gamma (storage dtype), colsum[n] = sum_k w_folded[n, k],
 *                  shift[n] = sum_k beta[k] w[n, k]   (fp32 [rows]); w is [rows, c] = torch Linear.weight
 * and AidGemmProblem.ln_* applies  rstd (x W'^T - mean colsum) + shift  in the GEMM epilogue.  Requirements as aid_layernorm. */
int aid_ln_stats(const void* x, float* stats, int64_t rows, int32_t c, float eps, int32_t dtype, void* stream);
int aid_ln_fold(const void* w, const void* gamma, const void* beta, void* w_folded, float* colsum, float* shift,
                int32_t rows, int32_t c, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Interpolated attention core on projected tensors.
 *   q   [n_frames, s, heads*d]        row stride ldq, frame stride q_fs   (elements)
 *   k   [n_kv,     l, heads*d]        row stride ldk, frame stride k_fs
 *   vt  [n_kv, heads*d, ldvt]         V TRANSPOSED (channel-major): vt[f][c][key]; ldvt >= l,
 *                                     ldvt % 8 == 0, frame stride vt_fs
 *   out [n_frames, s, heads*d]        row stride ldo, frame stride o_fs
 * Frame i attends with its own keys  K[kv_of(i)]  (kv_of = kv_map[i] if kv_map else i) and with
 * the end-point frames K[begin], K[end]:
 *   PLAIN : O_i = A(Q_i, K_i, V_i)
 *   INNER : Kc = (1-c_i) K[begin] + c_i K[end]  (same for V);
 *           O_i = fused ? A(Q_i, [K_i ; Kc], [V_i ; Vc]) : A(Q_i, Kc, Vc)
 *           Kc / Vc^T of the interior frames (0 < c_i < 1) are read from k2 / vt2, laid out like k / vt
 *           with one row per FRAME (frame strides k_fs / vt_fs); fill them with aid_lerp_kv() first.
 *   OUTER : O_i = (1-c_i) A(Q_i, [K_i;] K[begin], ..) + c_i A(Q_i, [K_i;] K[end], ..)
 * with A(Q,K,V) = softmax(Q K^T * softmax_scale) V per head, c_i = coef[i] (fp32, device).
 * A NEGATIVE coefficient marks frame i as PLAIN inside an INNER / OUTER launch: the unconditional half of a
 * classifier-free-guidance batch [cond frames ; uncond frames] then rides in the same call (begin / end must
 * index the cond half).  n_plain = number of such frames (host-side accounting only, may be 0).
 * Finally   out_i = (accumulate ? out_i : 0) + out_scale * (frame_scale ? frame_scale[i] : 1) * O_i.
 * Supported head dims d: 40, 64, 80, 160 (SD1.5 / SDXL).  No sequence-length restriction.
 * ------------------------------------------------------------------------------------- */
typedef struct AidAttnArgs {
    const void*    q;
    const void*    k;
    const void*    vt;
    void*          out;
    const float*   coef;         /* device [n_frames]; may be NULL for PLAIN                 */
    const float*   frame_scale;  /* device [n_frames] or NULL                                */
    const int32_t* kv_map;       /* device [n_frames] or NULL (identity)                     */
    const void*    k2;           /* INNER only: interpolated keys    [n_frames, l, heads*d]  */
    const void*    vt2;          /* INNER only: interpolated values^T [n_frames, heads*d, ldvt] */
    int32_t n_frames, n_kv;
    int32_t s, l, heads, d;
    int32_t ldq, ldk, ldvt, ldo;
    int64_t q_fs, k_fs, vt_fs, o_fs;
    int32_t mode;                /* AID_MODE_*                                               */
    int32_t fused;               /* 0/1: prepend the frame's own keys/values                 */
    int32_t begin, end;          /* end-point frame indices into k / vt                      */
    int32_t accumulate;          /* 0/1                                                      */
    int32_t dtype;               /* AID_DTYPE_*                                              */
    float   softmax_scale;       /* d^-0.5 for diffusers Attention                           */
    float   out_scale;
    int32_t n_plain;             /* frames with a negative coefficient (profiling accounting) */
    int32_t q_prescaled;         /* 1: q already holds q * softmax_scale * log2(e) (fold it into the     */
                                 /* q-projection via AidGemmProblem.scale); 0: the kernel scales Q itself */
    int32_t seg_executed;        /* profiling accounting: (frame, key segment) passes this launch really runs —  */
                                 /* fused END-POINT frames and coefficient-0/1 sides run fewer than the          */
                                 /* algorithmic count; 0 = unknown (reported equal to the algorithmic count)     */
    /* float32 precision of the two products of the core (AID_DTYPE_F32 only).  This is the field that was `reserved0`, which callers  */
    /* left zero: layout and ABI version are unchanged.  0 (a zeroed struct): exact fp32 products on v_mfma_f32_32x32x2_f32.            */
    /* 1 ("high"): the launch MAY form K Q'^T and V^T P^T from bfloat16 halves — the arithmetic of AidGemmProblem.f32_split,            */
    /*     Xh = bf16_rne(X),  Xl = bf16_rne(X - float(Xh)),   A B ~= Al Bh + Ah Bl + Ah Bh   (three v_mfma_f32_32x32x16_bf16, fp32 sums) */
    /* on Q' = Q * softmax_scale * log2(e), K, V^T and the unnormalised probabilities P; the softmax itself (maximum, exp2, row sum,    */
    /* rescale) stays unrounded fp32.  A score is then good to ~2^-16 of |q| |k| (not of the score): ~6e-6 - 8e-6 rel-L2 of the fp64     */
    /* output instead of ~3e-7.  A permission, never an error: a shape the split kernel does not run (or does not win on) stays on the   */
    /* exact kernel; aid_last_attn_variant() says which ran ("aid_attn_f32x3" / "aid_attn_f32").  Needs no workspace.  An infinite or    */
    /* over-range element gives NaN where the exact kernel gives inf.  AID_ERR_ARG: a value outside {0, 1}; non-zero with a 16-bit dtype. */
    int32_t f32_split;
    /* ABI v8 — additive score bias (NULL: none): diffusers' attention_mask after Attention.prepare_attention_mask, which every  */
    /* reference processor hands to get_attention_scores (interpolation.py:115-117, 604-606, 651, 738-739, 787):              */
    /*     scores = softmax_scale * Q K^T + bias        (baddbmm(attention_mask, q, k^T, beta = 1, alpha = scale))              */
    /* bias element (frame f, head h, query row r, key j) at  bias + f * bias_fs + h * bias_hs + r * bias_rs + j  (elements of    */
    /* the operand dtype; bias_hs = 0: one mask for all heads, bias_rs = 0: one row for all queries — the [B * H, 1, L] tensor   */
    /* of prepare_attention_mask is bias_fs = H * L, bias_hs = L, bias_rs = 0).  It covers ONE key segment of l keys: a call     */
    /* whose frames attend to [own ; end-point] keys (fused) is refused (AID_ERR_ARG) — the reference fails there too, at the    */
    /* broadcast of an l-wide mask against 2 l scores.  INNER / OUTER apply it to the begin, end and interpolated segments       */
    /* alike.  Strides are multiples of 1 element; the base pointer needs the operand dtype's alignment only.  v7's kv_padded    */
    /* (a layout promise no kernel depended on) is gone.                                                                         */
    /* Masks (values -10000, finfo.min, -inf; anything below -1e30 is read as -1e30).  Every kernel keeps the softmax reference   */
    /* of a row as (largest bias seen so far) + (reference of the rest) and adds a key's bias as its difference to the former,   */
    /* so the size of the mask value costs the scores of the live keys no bits:                                                  */
    /*   masked key in a row with a live key    weight exactly 0 for all three values, wherever the two sit — same 64-key tile,   */
    /*                                          an earlier or a later one;                                                        */
    /*   tile whose keys are all masked         adds exact zeros after a tile with a live key; in front of the first live key     */
    /*                                          (left padding, the first tiles of a row) it is accumulated and then cancelled     */
    /*                                          exactly (factor 2^-14427 or smaller = 0) when the live key arrives.  No NaN;      */
    /*   row whose keys are all masked          softmax(softmax_scale Q K^T) V over ALL its keys, for all three values: what the  */
    /*                                          reference computes for -10000 and, up to its own rounding of score + finfo.min   */
    /*                                          (uniform weights in fp16 / bf16), for finfo.min; for -inf the reference gives     */
    /*                                          NaN and this finite row stands in.  The row is a convex combination of V's rows. */
    const void* bias;
    int64_t bias_fs;
    int32_t bias_hs, bias_rs;
} AidAttnArgs;

int aid_attn_fwd(const AidAttnArgs* args /* host */, void* stream);

/* Interpolated keys / values for AID_MODE_INNER (reference interpolation.py:772-775):
 *   k2[i] = (1 - coef[i]) * k[begin] + coef[i] * k[end]     (and the same for vt -> vt2)
 * for every frame i with 0 < coef[i] < 1 (other frames are left untouched: the attention kernel reads
 * the end-point frames themselves).  k_fs / vt_fs are the frame strides in elements (multiples of 8)
 * of all four tensors.  The WHOLE stride of such a frame is written — k2[i * k_fs .. (i + 1) * k_fs) and
 * vt2[i * vt_fs .. (i + 1) * vt_fs), gap rows and V^T pad columns included, lerped from whatever k / vt
 * hold there — and all of k[begin], k[end], vt[begin], vt[end] is read.  One streaming launch. */
int aid_lerp_kv(const void* k, const void* vt, void* k2, void* vt2, const float* coef /* device */,
                int32_t n_frames, int32_t begin, int32_t end, int64_t k_fs, int64_t vt_fs, int32_t dtype,
                void* stream);

/* ---------------------------------------------------------------------------------------
 * IP-Adapter image attention over several key segments, accumulated into `out` in ONE launch — the image branches of diffusers'
 * IPAdapterAttnProcessor2_0 with several adapters per layer and / or regional ip_adapter_masks (no ABI version change: two new
 * entry points, this one and aid_processor_ip_fwd; no existing struct changes).  For every frame i, head h and query row s
 *     out[i, s, h d : (h + 1) d] = round( float(out[i, s, ...]) + sum_g scale_g * (w_g ? w_g[s] : 1) * softmax(Q K_g^T * softmax_scale) V_g )
 * over the n_segments <= AID_IP_MAX_SEGMENTS segments: every segment has its own softmax over its own t >= 1 keys, accumulation is
 * fp32 and the sum is rounded once.  Where aid_attn_fwd(accumulate = 1) adds one segment per launch (a pass over q and out each),
 * this reads q once, reads out once and writes it once; a zero scale_g or w_g[s] contributes exactly +-0.
 *   q, out  [n_frames, s, heads*d]   row strides ldq / ldo, frame strides q_fs / o_fs (elements)
 *   segment: k  [n_rows, t, heads*d] (row stride heads*d, frame stride k_fs), vt [n_rows, heads*d, ldvt] (V TRANSPOSED, frame stride
 *            vt_fs) — the layouts aid_gemm_nt writes for K = E Wk^T and V^T = Wv E^T; n_rows == n_frames (frame i uses row i) or
 *            n_rows == 1 (every frame uses row 0; k_fs / vt_fs are then not used); row_weight: device fp32 [s] or NULL.
 * Reads exactly: q[i, s', h d + c], out[i, s', h d + c] for s' < s, c < d; k[r, j, :heads*d] and vt[r, :heads*d, j] for j < t (rows
 * >= t of k, columns [t, ldvt) of vt, and everything between the strides never enter the arithmetic: they may hold NaN);
 * row_weight[0 .. s).  Writes exactly out[i, s', :heads*d].  q and out must not overlap.
 * Requirements: dtype f16 / bf16 (AID_DTYPE_F32: AID_ERR_DTYPE); d in {40, 64, 80, 160}, ldq / ldo / q_fs / o_fs / k_fs / vt_fs /
 * ldvt multiples of 8, ldq / ldo >= heads*d, ldvt >= t, q / out / k / vt 16-byte aligned, row_weight 4-byte aligned (AID_ERR_SHAPE);
 * NULL pointers, n_segments outside 1 .. AID_IP_MAX_SEGMENTS, t < 1, n_rows not 1 / n_frames, softmax_scale <= 0 without
 * q_prescaled (AID_ERR_ARG).  No allocation, no synchronisation.
 * ------------------------------------------------------------------------------------- */
#define AID_IP_MAX_SEGMENTS 8

typedef struct AidIpSegment {
    const void*  k;
    const void*  vt;
    const float* row_weight;     /* device fp32 [s] or NULL (= 1)                             */
    int64_t k_fs, vt_fs;         /* frame strides in elements                                 */
    int32_t t, ldvt, n_rows;
    float   scale;
} AidIpSegment;

typedef struct AidIpAttnArgs {
    const void* q;
    void*       out;
    const AidIpSegment* segments;   /* HOST array of n_segments entries                       */
    int32_t n_segments;
    int32_t n_frames, s, heads, d;
    int32_t ldq, ldo;
    int32_t dtype;               /* AID_DTYPE_F16 / AID_DTYPE_BF16                            */
    int64_t q_fs, o_fs;
    float   softmax_scale;       /* d^-0.5 for diffusers Attention                            */
    int32_t q_prescaled;         /* 1: q already holds q * softmax_scale * log2(e)            */
} AidIpAttnArgs;

int aid_ip_attn_fwd(const AidIpAttnArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * One whole processor call (what diffusers' Attention.forward hands to the AID processor):
 *   x   [n_frames, s, c]   hidden states          ctx [n_frames, l, cc] or NULL (self-attn: ctx = x)
 *   wq [c, c]  wk [c, cc]  wv [c, cc]  wo [c, c]  bo [c]      (torch Linear.weight layout [out, in])
 *   y   [n_frames, s, c]   = to_out( AID-attention( to_q(x), to_k(ctx), to_v(ctx) ) )
 * Launches: [1 LayerNorm or 1 row-statistics pass,] [LoRA: 1 down-projection GEMM,] 1 grouped GEMM (q, k, V^T [, K_ip, V_ip^T]), [INNER: 1 streaming K/V lerp,] 1 attention
 * kernel [+ 1 for the image branch, accumulating], [LoRA on to_out: 1 down-projection GEMM,] 1 GEMM (out-proj + bias [+ residual]).
 * Optional block-level fusion: with ln_eps > 0 the call computes on LayerNorm(x) (the block's
 * norm1 / norm2; self-attention keys / values use the normalised x too, a cross-attention ctx is left alone), and
 * with `residual` it returns  residual + to_out(...)  — together  h + attn(norm(h))  in one call.
 * `workspace` must hold aid_processor_workspace_bytes() bytes (16-byte aligned); it is
 * scratch, owned by the caller, and may be reused by the next call on the same stream.
 * ------------------------------------------------------------------------------------- */
typedef struct AidProcessorArgs {
    const void*  x;
    const void*  ctx;            /* NULL => self-attention                                   */
    const void*  wq;
    const void*  wk;
    const void*  wv;
    const void*  wo;
    const void*  bo;             /* NULL = no bias                                           */
    void*        y;
    const float* coef;           /* device [n_frames] (already rounded to the compute dtype, */
                                 /* interpolation.py:663); NULL for PLAIN                    */
    void*        workspace;
    size_t       workspace_bytes;
    int32_t n_frames, s, l, c, cc, heads;
    int32_t mode, fused;
    int32_t begin, end;          /* end-point frames (reference: 0 and n_frames-1)           */
    int32_t dtype;
    int32_t n_ctx;               /* number of ctx frames (n_frames, or fewer with ctx_map)   */
    const int32_t* ctx_map;      /* device [n_frames] frame -> ctx row, or NULL (identity)   */
    int32_t n_plain;             /* frames whose coef is negative (PLAIN riders), accounting  */
    float   ln_eps;              /* > 0: LayerNorm(x) over c first (gamma / beta below)       */
    const void* ln_gamma;        /* [c] or NULL                                               */
    const void* ln_beta;         /* [c] or NULL                                               */
    const void* residual;        /* [n_frames, s, c] or NULL: added to y (may alias x)        */
    /* ---- IP-Adapter image branch (ip == NULL: none).  Image tokens: n_ip rows of [t_ip, cc] (cc = the text   */
    /* context width), row r at ip + r * ip_stride elements (a strided view such as ip_hidden_states[0][::3]    */
    /* needs no copy).  K_ip = to_k_ip(ip), V_ip = to_v_ip(ip) are projected in the same grouped launch as      */
    /* q / k / V^T; frame i uses image row ip_map[i] (NULL = identity, then n_ip == number of AID frames).      */
    /*   AID_IP_SAME       O += ip_scale * [the text mode's interpolation scheme on the image keys]             */
    /*                     (OUTER only: interpolation.py:329-367, outputs are lerped AFTER the sum)             */
    /*   AID_IP_PLAIN      O += ip_scale * A(Q_i, K_ip[row i], V_ip[row i])      (interpolation.py:525-530;     */
    /*                     de-activated IPAdapterAttnProcessor2_0 with the [9,1,T,Cc] fold as t_ip = 3 T)       */
    /* ip_frame_scale (device [n_frames] or NULL) multiplies ip_scale per frame: ScaleControlIPAttnProcessor's     */
    /* `coef * ip_hidden_states` (interpolation.py:146-150, 196) is AID_IP_PLAIN with ip_frame_scale = coef.       */
    const void*    ip;
    const void*    wk_ip;        /* [c, cc] */
    const void*    wv_ip;        /* [c, cc] */
    const int32_t* ip_map;       /* device [n_frames] or NULL */
    const float*   ip_frame_scale; /* device [n_frames] or NULL */
    int64_t ip_stride;           /* elements between consecutive image rows (>= t_ip * cc, multiple of 8) */
    int32_t n_ip, t_ip;
    int32_t ip_mode;             /* AID_IP_*                                                  */
    float   ip_scale;
    int32_t ip_begin, ip_end;    /* AID_IP_SAME: image rows of the end-point frames           */
    int32_t seg_executed;        /* accounting, see AidAttnArgs.seg_executed (text launch only) */
    /* float32 precision of the attention core's two products: AidAttnArgs.f32_split, same values, same errors, copied into every     */
    /* attention launch of the call (text branch, image branch).  Independent of f32_split below (the projections).  This is the slot  */
    /* that was reserved2 (v6 / v7: kv_cached_lt, removed in v8), which callers left zero: zero = exact, as before.                    */
    int32_t f32_attn_split;
    /* ---- folded LayerNorm (ln_eps > 0 and ln_wq != NULL): the call runs aid_ln_stats on x instead of aid_layernorm and  */
    /* projects x with the folded weights (aid_ln_fold of wq / wk / wv with ln_gamma / ln_beta; wk / wv only for           */
    /* self-attention, a cross-attention ctx is not normalised).  ln_const: fp32 [6, c] = colsum_q, shift_q, colsum_k,     */
    /* shift_k, colsum_v, shift_v.  Needs c % 64 == 0 (the projections then run on the k % 64 == 0 engines).               */
    const void*  ln_wq;
    const void*  ln_wk;
    const void*  ln_wv;
    const float* ln_const;
    /* ---- step-invariant keys / values of a cross-attention layer (ABI v5; both NULL: project them in this call).  The text  */
    /* context does not change over the denoising loop (reference pipeline_interpolated_sd.py:1859-1867 hands the same       */
    /* prompt_embeds to every step), so K = to_k(ctx) [n_ctx, l, c] and V^T = Wv ctx^T [n_ctx, c, round_up(l, 8)] can be      */
    /* projected ONCE per (layer, context) with aid_gemm_nt and handed to every later call: the grouped launch then holds     */
    /* the query projection alone.  Only valid with ctx != NULL; the caller owns the buffers and their validity.             */
    const void*  k_cached;
    const void*  vt_cached;
    int32_t      cu_share;       /* ABI v7: see AidGemmProblem.cu_share — handed to every GEMM launch of the call            */
    /* float32 matmul precision of every projection GEMM the call launches (q / k / v / out, the image-token k / v, the LoRA down     */
    /* projections): AidGemmProblem.f32_split, same values, same errors (the field that was reserved1: zero = exact, as before).      */
    /* The attention core's two products have their own switch: f32_attn_split above.                                                  */
    int32_t      f32_split;
    /* ABI v8: additive score bias of the text attention (attention_mask), see AidAttnArgs.bias; not with `fused`, not with `ip` */
    const void*  attn_bias;
    int64_t      attn_bias_fs;
    int32_t      attn_bias_hs, attn_bias_rs;
    /* ---- ABI v9: unmerged LoRA adapters of the four projections (all ranks 0: none).  Projection p in {q, k, v, o} with    */
    /* lora_r_p > 0 computes  in W_p^T + U_p B_p^T  with  U_p = round(in A_p^T)  (`in` = its input: x, ctx or the attention    */
    /* output o), where A_p [lora_r_p, in width] holds the adapters' lora_A weights stacked by rows, each multiplied by its   */
    /* scaling, and B_p = lora_up_p [c, lora_r_p] their lora_B weights side by side (ranks zero-padded to a multiple of 64,   */
    /* <= 512).  The down weights are stacked per input tensor, so that each input is read once:                             */
    /*   lora_down_x   [r_q (+ r_k + r_v for self-attention), c]   rows A_q; A_k; A_v                                        */
    /*   lora_down_ctx [r_k + r_v, cc]                             rows A_k; A_v   (cross-attention)                         */
    /*   lora_down_o   [r_o, c]                                                                                             */
    /* One extra GEMM launch projects x (and ctx) down, one o; U lives in the workspace (aid_processor_workspace_bytes grows  */
    /* by it; unchanged with every rank 0).  Refused (AID_ERR_ARG): with ln_wq (the folded LayerNorm; pass ln_eps with        */
    /* ln_wq = NULL instead), LoRA on k / v with k_cached (cached keys must already hold the adapter term).                   */
    const void*  lora_down_x;
    const void*  lora_down_ctx;
    const void*  lora_down_o;
    const void*  lora_up_q;
    const void*  lora_up_k;
    const void*  lora_up_v;
    const void*  lora_up_o;
    int32_t      lora_r_q;
    int32_t      lora_r_k;
    int32_t      lora_r_v;
    int32_t      lora_r_o;
    /* ---- ABI v10: DoRA.  lora_gain_p (fp32 [c], NULL: none; only with lora_r_p > 0, else AID_ERR_ARG) is the row gain of      */
    /* projection p's adapter (aid_dora_gain): the projection computes  gain_p o (in W_p^T + U_p B_p^T)  (AidGemmProblem.         */
    /* lr_row_scale, with the side of the form the call plans for that projection).  The down projections U are unchanged.        */
    const float* lora_gain_q;
    const float* lora_gain_k;
    const float* lora_gain_v;
    const float* lora_gain_o;
} AidProcessorArgs;

size_t aid_processor_workspace_bytes(const AidProcessorArgs* args /* host */);
int    aid_processor_fwd(const AidProcessorArgs* args /* host */, void* stream);
/* The same call with IMAGE SEGMENTS: n_ip_segs entries of AidIpSegment (a HOST array; more than AID_IP_MAX_SEGMENTS run as several
 * launches) are added to the attention output by aid_ip_attn_fwd on the call's q / o workspace, after the text attention and before
 * the out projection — several IP-Adapters per layer, regional masks (AidIpSegment.row_weight); each segment's K / V^T is projected
 * by the caller (aid_gemm_nt; they do not change over the denoising loop).  AidProcessorArgs itself is unchanged (and so are the ABI
 * version and aid_processor_workspace_bytes): the segments travel beside it.  n_ip_segs == 0 is aid_processor_fwd.  With segments the
 * call must be a cross-attention PLAIN call with ip == NULL (AID_ERR_ARG) in a 16-bit dtype (AID_ERR_DTYPE); attn_bias is ALLOWED and
 * covers the text launch only, as diffusers' IPAdapterAttnProcessor2_0 masks the text scores only.  LoRA / DoRA on the four
 * projections, k_cached, LayerNorm and residual work as without segments.  Segment errors as aid_ip_attn_fwd; everything is checked
 * before the first launch. */
int    aid_processor_ip_fwd(const AidProcessorArgs* args /* host */, const AidIpSegment* ip_segs /* host */, int32_t n_ip_segs, void* stream);

/* ---------------------------------------------------------------------------------------
 * End-point K / V^T store (no ABI version change: three new entry points, no existing struct changes).  The two end-point frames of
 * an AID run need nothing from the interior frames (with coefficient 0 / 1 every mode is plain attention of that frame), so their
 * self-attention keys / values per (layer, AID step) can be RECORDED in one run and further interior frames rendered against them in
 * later runs whose batch holds the new frames only (REPLAY).  A store of one layer:
 *   k_store  [n_steps, 2, k_fs]    vt_store [n_steps, 2, vt_fs]      (entry 0 = begin frame, 1 = end frame; element type of the call)
 * aid_endpoint_rows moves, in ONE streaming launch, the four contiguous blocks k[row_begin], k[row_end] (k_fs elements each) and
 * vt[row_begin], vt[row_end] (vt_fs elements each; rows are k_fs / vt_fs apart) between a call's k / vt tensors and slot *step:
 *   AID_EP_PUT  reads  k[row_begin * k_fs .. + k_fs), k[row_end * k_fs .. + k_fs), vt[row_begin * vt_fs .. + vt_fs),
 *                      vt[row_end * vt_fs .. + vt_fs) and *step;
 *               writes k_store[(2 * *step + e) * k_fs .. + k_fs), vt_store[(2 * *step + e) * vt_fs .. + vt_fs) for e = 0, 1
 *   AID_EP_GET  reads what PUT writes (and *step), writes what PUT reads.  Nothing else is read or written.
 * The whole block moves — gap rows and V^T pad columns included, as aid_lerp_kv lerps them.  `step` is a DEVICE pointer read by the
 * kernel, like the coefficient buffers: a launch captured into a graph addresses another slot at every replay with no node update.
 * A *step outside [0, n_steps) moves nothing (a memory-safety guard, not a mode: the host keeps the index in range).
 * Requirements as aid_lerp_kv: k_fs / vt_fs positive multiples of 8, k / vt / k_store / vt_store 16-byte aligned (AID_ERR_SHAPE);
 * f16 / bf16 / f32 (AID_ERR_DTYPE); NULL pointers, step not 4-byte aligned, negative rows, n_steps < 1, a direction other than
 * PUT / GET (AID_ERR_ARG) — all before any launch.  16-byte vector loads and stores on a grid-stride walk; no atomics, no LDS.
 * ------------------------------------------------------------------------------------- */
#define AID_EP_PUT 0          /* call  -> store */
#define AID_EP_GET 1          /* store -> call  */

typedef struct AidEndpointRows {
    void*          k;            /* [rows, k_fs]  of the call                                  */
    void*          vt;           /* [rows, vt_fs] of the call                                  */
    void*          k_store;      /* [n_steps, 2, k_fs]                                         */
    void*          vt_store;     /* [n_steps, 2, vt_fs]                                        */
    const int32_t* step;         /* DEVICE: the slot index, read by the kernel                 */
    int64_t k_fs, vt_fs;         /* block sizes = row strides, in elements                     */
    int32_t row_begin, row_end;  /* rows of k / vt                                             */
    int32_t n_steps;
    int32_t direction;           /* AID_EP_PUT / AID_EP_GET                                    */
    int32_t dtype;               /* AID_DTYPE_*                                                */
} AidEndpointRows;

int aid_endpoint_rows(const AidEndpointRows* args /* host */, void* stream);

/* aid_processor_fwd with the store of its layer beside it (AidProcessorArgs is unchanged).  ep == NULL is aid_processor_fwd.
 *   AID_EP_RECORD  exactly aid_processor_fwd(args) plus one AID_EP_PUT of rows args->begin / args->end of the call's k / V^T behind
 *                  the projection launch: y is bit-identical, aid_processor_ep_workspace_bytes == aid_processor_workspace_bytes.
 *   AID_EP_REPLAY  `args` describes the LOCAL frames only — interior frames (0 < coef < 1) and PLAIN riders (negative coef).  The
 *                  workspace gives k / V^T two rows more than n_frames: the projections fill rows 0 .. n_frames - 1, one AID_EP_GET
 *                  fills rows n_frames (begin) and n_frames + 1 (end), and the rest of the call — the lerp of INNER, every attention
 *                  kernel, the out projection, the epilogues — runs unchanged with begin = n_frames, end = n_frames + 1.
 *                  args->begin / args->end are not read.
 * The store's blocks are k_fs = s * c and vt_fs = c * round_up(s, 8) elements of args->dtype.  Both modes are self-attention AID
 * calls: ctx != NULL, mode == AID_MODE_PLAIN, ip != NULL, a NULL store pointer, n_steps < 1 or a mode other than RECORD / REPLAY is
 * AID_ERR_ARG, a misaligned store AID_ERR_SHAPE — checked, with everything aid_processor_fwd checks, before the first launch.
 * LoRA / DoRA, attn_bias, LayerNorm (folded or not), residual, f32_split / f32_attn_split work as in aid_processor_fwd: it is the
 * same code path.  Cross-attention needs no store: the end points' text contexts are loop-invariant, a replay call appends them to
 * ctx and points ctx_map / begin / end of aid_processor_fwd at them. */
#define AID_EP_RECORD 1
#define AID_EP_REPLAY 2

typedef struct AidEndpointStore {
    void*          k_store;      /* [n_steps, 2, s * c]                                        */
    void*          vt_store;     /* [n_steps, 2, c * round_up(s, 8)]                           */
    const int32_t* step;         /* DEVICE: the AID step of this call                          */
    int32_t n_steps;
    int32_t mode;                /* AID_EP_RECORD / AID_EP_REPLAY                              */
} AidEndpointStore;

size_t aid_processor_ep_workspace_bytes(const AidProcessorArgs* args /* host */, const AidEndpointStore* ep /* host */);
int    aid_processor_ep_fwd(const AidProcessorArgs* args /* host */, const AidEndpointStore* ep /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Key-frame K / V^T store (no ABI version change: three new entry points, no existing struct changes).  An end point's trajectory
 * depends on neither its partner nor the AID mode nor the fusion flag — it is plain attention of that frame — so ONE recording per
 * KEY FRAME serves every pair that contains the frame, in both directions, and every early mode.  A key-frame store of one layer holds
 * one frame, half of the pair slot above; every key frame has its own allocation:
 *   k_store  [n_steps, k_fs]    vt_store [n_steps, vt_fs]      (element type of the call)
 * aid_keyframe_rows moves, in ONE streaming launch, n_rows (1 .. AID_KF_MAX_ROWS) rows between a call's k / vt tensors and as many
 * stores (`rows` is a HOST array; its entries travel by value in the kernel arguments).  For entry i:
 *   AID_KF_PUT  reads  k[row_i * k_fs .. + k_fs), vt[row_i * vt_fs .. + vt_fs) and *step;
 *               writes k_store_i[*step * k_fs .. + k_fs), vt_store_i[*step * vt_fs .. + vt_fs)
 *   AID_KF_GET  reads what PUT writes (and *step), writes what PUT reads.  Nothing else is read or written.
 * The whole block moves — gap rows and V^T pad columns included, exactly as aid_endpoint_rows moves them.  `step` is a DEVICE pointer
 * read by the kernel: a launch captured into a graph addresses another slot at every replay with no node update.  A *step outside
 * [0, n_steps) moves nothing (a memory-safety guard, not a mode: the host keeps the index in range).
 * Requirements as aid_endpoint_rows: k_fs / vt_fs positive multiples of 8, k / vt and every k_store / vt_store 16-byte aligned
 * (AID_ERR_SHAPE); f16 / bf16 / f32 (AID_ERR_DTYPE); NULL pointers (rows and every store included), step not 4-byte aligned, n_rows
 * outside 1 .. AID_KF_MAX_ROWS, a negative row, n_steps < 1, a direction other than PUT / GET (AID_ERR_ARG) — all before any launch.
 * 16-byte vector loads and stores on a grid-stride walk; no atomics, no LDS.
 * ------------------------------------------------------------------------------------- */
#define AID_KF_MAX_ROWS 8
#define AID_KF_PUT 0          /* call  -> store */
#define AID_KF_GET 1          /* store -> call  */

typedef struct AidKeyframeRow {
    void*   k_store;             /* [n_steps, k_fs]   of ONE key frame                         */
    void*   vt_store;            /* [n_steps, vt_fs]                                           */
    int32_t row;                 /* row of the call's k / vt                                   */
} AidKeyframeRow;

typedef struct AidKeyframeRows {
    void*                 k;     /* [rows, k_fs]  of the call                                  */
    void*                 vt;    /* [rows, vt_fs] of the call                                  */
    const AidKeyframeRow* rows;  /* HOST: n_rows entries                                       */
    const int32_t*        step;  /* DEVICE: the slot index, read by the kernel                 */
    int64_t k_fs, vt_fs;         /* block sizes = row strides, in elements                     */
    int32_t n_rows;              /* 1 .. AID_KF_MAX_ROWS                                       */
    int32_t n_steps;
    int32_t direction;           /* AID_KF_PUT / AID_KF_GET                                    */
    int32_t dtype;               /* AID_DTYPE_*                                                */
} AidKeyframeRows;

int aid_keyframe_rows(const AidKeyframeRows* args /* host */, void* stream);

/* aid_processor_fwd with key-frame stores of its layer beside it (AidProcessorArgs is unchanged).  kf == NULL is aid_processor_fwd.
 *   AID_KF_RECORD  `args` is a PLAIN self-attention call (ctx == NULL, ip == NULL, mode == AID_MODE_PLAIN) over a batch that holds the
 *                  key frames; `rows` has 1 .. AID_KF_MAX_ROWS entries with distinct rows < n_frames.  Exactly aid_processor_fwd(args)
 *                  plus one AID_KF_PUT of those rows of the call's k / V^T behind the projection launch: y is bit-identical,
 *                  aid_processor_kf_workspace_bytes == aid_processor_workspace_bytes.
 *   AID_KF_REPLAY  `rows` has exactly TWO entries: entry 0 the begin frame's store, entry 1 the end frame's (`row` is ignored).
 *                  `args` describes the LOCAL frames only, with an AID mode, as in AID_EP_REPLAY: the workspace gives k / V^T two rows
 *                  more than n_frames, one AID_KF_GET fills rows n_frames (begin) and n_frames + 1 (end) from the two stores, and the
 *                  rest of the call runs unchanged with begin = n_frames, end = n_frames + 1 (args->begin / args->end are not
 *                  read).  It IS the AID_EP_REPLAY path — only the copy launch that fills the two rows differs — and
 *                  aid_processor_kf_workspace_bytes equals aid_processor_ep_workspace_bytes of a replay.  Swapping the two entries
 *                  renders the reverse direction.
 * The stores' blocks are k_fs = s * c and vt_fs = c * round_up(s, 8) elements of args->dtype.  ctx != NULL, ip != NULL, RECORD on an
 * AID call, REPLAY on a PLAIN call, REPLAY with n_rows != 2, a duplicate or out-of-range row in RECORD, NULL rows / store / step
 * pointers, n_steps < 1 or a mode other than RECORD / REPLAY is AID_ERR_ARG, a misaligned store AID_ERR_SHAPE — checked, with
 * everything aid_processor_fwd checks, before the first launch.  LoRA / DoRA, attn_bias, LayerNorm (folded or not), residual,
 * f32_split / f32_attn_split work as in aid_processor_fwd: it is the same code path. */
#define AID_KF_RECORD 1
#define AID_KF_REPLAY 2

typedef struct AidKeyframeCall {
    const AidKeyframeRow* rows;  /* HOST: n_rows entries (RECORD: 1 .. AID_KF_MAX_ROWS; REPLAY: 2) */
    const int32_t*        step;  /* DEVICE: the AID step of this call                          */
    int32_t n_rows;
    int32_t n_steps;
    int32_t mode;                /* AID_KF_RECORD / AID_KF_REPLAY                              */
} AidKeyframeCall;

size_t aid_processor_kf_workspace_bytes(const AidProcessorArgs* args /* host */, const AidKeyframeCall* kf /* host */);
int    aid_processor_kf_fwd(const AidProcessorArgs* args /* host */, const AidKeyframeCall* kf /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Key-frame store in 8-bit blocks, "q8" (no ABI version change: four new entry points, no existing struct, constant or entry point
 * changes).  LOSSY and opt-in: a key frame's K / V^T are written once and read many times, and enter a replay only as the two
 * end-point key segments.  A *block row* of n elements (one k block, n = k_fs, or one V^T block, n = vt_fs; n a positive multiple of
 * 8) is stored as aid_q8_block_bytes(n) = round_up(n + ceil(n / 32), 16) bytes:
 *   bytes [0, n)                    int8 elements
 *   bytes [n, n + ceil(n / 32))     one exponent byte per block of 32 consecutive elements (the last block may hold 8, 16 or 24)
 *   the rest up to the 16-byte boundary is never read and never written.
 * Stored elements: every element of a k block; of a V^T block — vt_fs / vt_ld rows of vt_ld columns — the first vt_cols columns of
 * every row.  Columns >= vt_cols are pad: they are never read into arithmetic (they may hold NaN), their int8 is 0, they take no part
 * in a block's maximum, and GET writes +0 there (nothing reads those columns: the contract of aid_attn_fwd).
 * Per block, with a = max |x| over its stored elements (exact, in fp32): e is the smallest integer with 127 * 2^e >= a, clamped to
 * [-126, 120] (-126 when a == 0 or the block stores nothing); the exponent byte is e + 127; every element is
 * q = clamp(rne(x * 2^-e), -127, 127), round-half-to-even, the product exact in fp32.  The value that comes back is q * 2^e converted
 * to the element type — exact in f16, bf16 and f32 — so |y - x| <= 2^(e-1) < a / 127 for every stored element, and a block of f16
 * subnormals comes back unchanged.  Non-finite stored elements are outside the contract: the values that come back are unspecified,
 * the bytes read and written are the ones stated.
 * aid_keyframe_rows_q8 is aid_keyframe_rows with such stores, k_store_i [n_steps, aid_q8_block_bytes(k_fs)] and vt_store_i
 * [n_steps, aid_q8_block_bytes(vt_fs)] bytes, in ONE streaming launch.  For entry i, with B(n) = n + ceil(n / 32):
 *   AID_KF_PUT  reads  k[row_i * k_fs .. + k_fs), vt[row_i * vt_fs .. + vt_fs) and *step;
 *               writes bytes [0, B(k_fs)) of block row *step of k_store_i and bytes [0, B(vt_fs)) of block row *step of vt_store_i
 *   AID_KF_GET  reads what PUT writes (and *step), writes what PUT reads.  Nothing else is read or written.
 * A *step outside [0, n_steps) moves nothing.  Everything aid_keyframe_rows checks is checked; in addition vt_ld % 8 != 0,
 * vt_fs % vt_ld != 0 or vt_cols outside 1 .. vt_ld is AID_ERR_SHAPE, and the stores are 16-byte aligned (AID_ERR_SHAPE) — all before
 * any launch.  A lane moves one 16-byte chunk of the call tensor and 8 (f16 / bf16) or 4 (f32) store bytes; the 4 or 8 lanes of a block
 * agree on its maximum by lane exchange; no atomics, no LDS.
 * aid_processor_kf_q8_fwd is aid_processor_kf_fwd with that launch as the copy step (vt_ld = round_up(s, 8), vt_cols = s): RECORD —
 * y bit-identical to aid_processor_fwd, the call's k / V^T not modified, the workspace equal; REPLAY — rows n_frames / n_frames + 1
 * are filled by the dequantising GET (pad columns +0), the rest of the call is unchanged.  Every refusal of aid_processor_kf_fwd
 * applies; aid_processor_kf_q8_workspace_bytes == aid_processor_kf_workspace_bytes.  f16 / bf16 / f32.
 * ------------------------------------------------------------------------------------- */
size_t aid_q8_block_bytes(int64_t n_elements);      /* 0 for n < 8 or n % 8 != 0 */

typedef struct AidKeyframeRowsQ8 {
    void*                 k;     /* [rows, k_fs]  of the call, element type `dtype`            */
    void*                 vt;    /* [rows, vt_fs] of the call                                  */
    const AidKeyframeRow* rows;  /* HOST: n_rows entries; k_store / vt_store are q8 stores:    */
                                 /*   [n_steps, aid_q8_block_bytes(k_fs | vt_fs)] bytes        */
    const int32_t*        step;  /* DEVICE: the slot index, read by the kernel                 */
    int64_t k_fs, vt_fs;         /* block sizes = row strides of the call, in elements         */
    int32_t vt_ld, vt_cols;      /* V^T rows of vt_ld columns, the first vt_cols stored        */
    int32_t n_rows;              /* 1 .. AID_KF_MAX_ROWS                                       */
    int32_t n_steps;
    int32_t direction;           /* AID_KF_PUT / AID_KF_GET                                    */
    int32_t dtype;               /* AID_DTYPE_*                                                */
} AidKeyframeRowsQ8;

int    aid_keyframe_rows_q8(const AidKeyframeRowsQ8* args /* host */, void* stream);
size_t aid_processor_kf_q8_workspace_bytes(const AidProcessorArgs* args /* host */, const AidKeyframeCall* kf /* host */);
int    aid_processor_kf_q8_fwd(const AidProcessorArgs* args /* host */, const AidKeyframeCall* kf /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Corner-weighted AID: interpolation among up to AID_MAX_CORNERS end points, in the LIVE form — the corner frames sit in the batch, as
 * the two end points of aid_attn_fwd do (no ABI version change: five new entry points, no existing struct, constant or entry point
 * changes; no stores).  Corners are rows r_0 .. r_{M-1} of k / vt (frame rows, or context rows when kv_map / ctx_map is given;
 * duplicates allowed), 1 <= M <= AID_MAX_CORNERS.  Frame i has an fp32 weight row w[i, 0 .. M), non-negative, in a DEVICE tensor
 * [n_frames, M] read by the kernels, like the coefficient buffers: a captured graph reads live values.
 *   OUTER : O_i = sum_m w[i, m] * A(Q_i, [K_i ;] K[r_m], [V_i ;] V[r_m])
 *   INNER : Kc_i = sum_m w[i, m] * K[r_m]   (same for V);   O_i = A(Q_i, [K_i ;] Kc_i, [V_i ;] Vc_i)
 * with [K_i ;] present when `fused` and A as in aid_attn_fwd.  The last n_plain frames of a call are PLAIN riders (O_i = A(Q_i, K_i, V_i));
 * here n_plain is AUTHORITATIVE and the riders' weight rows are not read.  M = 2 with w = (1 - c, c) is aid_attn_fwd's OUTER / INNER.
 *
 * aid_mix_kv — the INNER mix, one streaming launch:
 *   k2[i] = sum_m w[i, m] * k[rows[m]]    vt2[i] = sum_m w[i, m] * vt[rows[m]]       for i in [0, n_frames - n_plain)
 * Products and sum in fp32, in corner order, one rounding to the storage type; a term with weight exactly 0 is skipped, so a one-hot
 * row returns the corner's bits (f32 storage carries the rounding errors of the sum along and adds them before the final rounding).
 * k_fs / vt_fs are the row strides in elements of all four tensors.  Reads exactly k[rows[m] * k_fs .. + k_fs) and
 * vt[rows[m] * vt_fs .. + vt_fs) for every m — each ONCE per launch, whatever n_frames is — and w[i, 0 .. M) for i < n_frames - n_plain.
 * Writes exactly k2[i * k_fs .. + k_fs) and vt2[i * vt_fs .. + vt_fs) for i < n_frames - n_plain: the whole stride of a mixed frame,
 * gap rows and V^T pad columns included, mixed from whatever k / vt hold there, exactly as aid_lerp_kv does; the riders' rows of
 * k2 / vt2 are untouched.  `rows` is a HOST array (its entries travel by value in the kernel arguments).
 * AID_ERR_ARG: a NULL pointer, n_corners outside 1 .. AID_MAX_CORNERS, a negative row, n_frames < 1, n_plain outside [0, n_frames];
 * AID_ERR_SHAPE: k_fs / vt_fs not positive multiples of 8, k / vt / k2 / vt2 not 16-byte aligned, weights not 4-byte aligned;
 * AID_ERR_DTYPE — all before any launch.  16-byte vector loads and stores on a grid-stride walk; no LDS, no atomics.
 *
 * aid_attn_corners_fwd — aid_attn_fwd among the corners.  AidAttnArgs is unchanged; its coef, begin, end, frame_scale, accumulate and
 * out_scale are NOT read, mode is AID_MODE_INNER or AID_MODE_OUTER (PLAIN: AID_ERR_ARG).  One small launch first fills the PAIR TABLE
 * in `scratch` (caller-owned device memory, 16-byte aligned, aid_corners_scratch_bytes(n_frames, n_corners) bytes; too small:
 * AID_ERR_WORKSPACE) from the weights: for pass p = 0 .. ceil(M / 2) - 1, with a = w[i, 2p], b = (2p + 1 < M) ? w[i, 2p + 1] : 0,
 * s = a + b:   coef_p[i] = s > 0 ? b / s : 0,   scale_p[i] = s;   riders: coef = -1, scale = 1   (no division by zero, no NaN).
 *   INNER  aid_mix_kv into the caller's k2 / vt2, then ONE aid_attn_fwd whose coefficient is 0.5 for every AID frame and -1 for the
 *          riders: every AID frame reads its k2 / vt2 row.
 *   OUTER  pass 0 is aid_attn_fwd over all frames with begin = r_0, end = r_1 (r_0 when M = 1), coef_0, frame_scale = scale_0,
 *          accumulate = 0; pass p >= 1 runs over the first n_frames - n_plain frames with begin = r_2p, end = r_2p+1, coef_p,
 *          frame_scale = scale_p, accumulate = 1.  A lone last corner is the pair (r, r) with coefficient 0.  Each accumulating pass
 *          rounds `out` once more in its storage type.
 * Every refusal of aid_attn_fwd applies (a `bias` with `fused` included); a corner row >= n_kv, n_plain outside [0, n_frames] and
 * every NULL pointer of AidCorners is AID_ERR_ARG; weights not 4-byte / scratch not 16-byte aligned AID_ERR_SHAPE — all before any launch.
 *
 * aid_processor_corners_fwd — aid_processor_fwd with its attention step replaced by that composition; the pair table (and, for
 * INNER, k2 / vt2) are carved from the workspace, which must hold aid_processor_corners_workspace_bytes() bytes
 * (AidCorners.scratch is not read).  args->coef / begin / end are not read.  corners == NULL is aid_processor_fwd.  mode == PLAIN,
 * ip != NULL, a corner row >= the number of k / V^T rows: AID_ERR_ARG, with everything aid_processor_fwd checks, before the first
 * launch.  LoRA / DoRA, LayerNorm (folded or not), residual, f32_split / f32_attn_split, attn_bias (not with fused) and cached text
 * K / V work as in aid_processor_fwd: it is the same code path.
 * ------------------------------------------------------------------------------------- */
#define AID_MAX_CORNERS 8

typedef struct AidCorners {
    const int32_t* rows;         /* HOST: n_corners rows of k / vt                             */
    const float*   weights;      /* DEVICE fp32 [n_frames, n_corners], read by the kernels     */
    void*          scratch;      /* DEVICE: the pair table (aid_attn_corners_fwd only)         */
    size_t         scratch_bytes;
    int32_t        n_corners;    /* 1 .. AID_MAX_CORNERS                                       */
} AidCorners;

int    aid_mix_kv(const void* k, const void* vt, void* k2, void* vt2, const int32_t* rows /* host */, const float* weights /* device */,
                  int32_t n_frames, int32_t n_plain, int32_t n_corners, int64_t k_fs, int64_t vt_fs, int32_t dtype, void* stream);
size_t aid_corners_scratch_bytes(int32_t n_frames, int32_t n_corners);      /* 0 for n_frames < 1 or n_corners outside 1 .. 8 */
int    aid_attn_corners_fwd(const AidAttnArgs* args /* host */, const AidCorners* corners /* host */, void* stream);
size_t aid_processor_corners_workspace_bytes(const AidProcessorArgs* args /* host */, const AidCorners* corners /* host */);
int    aid_processor_corners_fwd(const AidProcessorArgs* args /* host */, const AidCorners* corners /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Key-frame blend: a corner-weighted call whose corners are RECORDED key frames — the store form of the section above (no ABI version
 * change: three new entry points and one struct; no existing struct, constant or entry point changes).  Corner m is block row *step
 * of key frame m's store (AidKeyframeRow.k_store / vt_store, `row` ignored; the same store may stand twice), 1 <= M <= AID_MAX_CORNERS
 * = AID_KF_MAX_ROWS.  Native stores ([n_steps, k_fs] / [n_steps, vt_fs] elements of the call dtype, q8 == 0) or 8-bit block stores
 * ([n_steps, aid_q8_block_bytes(.)] bytes, q8 == 1) as aid_keyframe_rows / aid_keyframe_rows_q8 PUT leaves them.  `weights` is
 * AidCorners.weights: DEVICE fp32 [n_frames, M], read by the kernels, the riders' rows not read.
 *
 * aid_mix_kv_stores — the INNER mix read straight from the stores, one streaming launch:
 *   k2[i] = sum_m w[i, m] * K_m[*step]    vt2[i] = sum_m w[i, m] * V^T_m[*step]       for i in [0, n_frames - n_plain)
 * It is aid_keyframe_rows[_q8] GET of the M rows followed by aid_mix_kv on them, bit for bit, without the M rows in between: the
 * arithmetic is aid_mix_kv's (fp32 products and sum in corner order, one rounding; a weight of exactly 0 is skipped, so a one-hot row
 * returns the corner's bits — for q8 the dequantised ones — and a skipped corner's block may hold anything; f32 storage carries the
 * rounding errors along).  A q8 value is q * 2^e as GET rounds it to the call dtype; V^T pad columns (column >= vt_cols of a row of
 * vt_ld) of q8 stores enter as +0, so they are +0 in every mixed row.
 * Reads exactly block row *step of every store — [*step * k_fs .. + k_fs) elements (native) or bytes [0, n + ceil(n / 32)) of the
 * block row (q8), each ONCE per launch — the one int32 *step, and w[i, 0 .. M) for i < n_frames - n_plain.  Writes exactly
 * k2[i * k_fs .. + k_fs) and vt2[i * vt_fs .. + vt_fs) for i < n_frames - n_plain: whole blocks, gap rows and pad columns included; the
 * riders' rows are untouched.  A *step outside [0, n_steps) writes nothing.  n_plain == n_frames launches nothing.
 * AID_ERR_ARG: b, rows, a store, step, weights, k2 or vt2 NULL, n_corners outside 1 .. AID_MAX_CORNERS, n_steps < 1, q8 outside
 * {0, 1}, n_frames < 1, n_plain outside [0, n_frames], step not 4-byte aligned; AID_ERR_DTYPE; AID_ERR_SHAPE: k_fs / vt_fs not
 * positive multiples of 8, for q8 vt_ld % 8 != 0, vt_ld < 8, vt_fs % vt_ld != 0 or vt_cols outside [1, vt_ld] (vt_ld / vt_cols are
 * not read for native stores), k2 / vt2 / a store not 16-byte aligned, weights not 4-byte aligned — all before any launch.
 * 16-byte vector stores on a grid-stride walk; no LDS, no atomics.
 *
 * aid_processor_kf_blend_fwd — aid_processor_corners_fwd whose corners are recorded key frames.  `args` describes the LOCAL frames
 * only (the AID frames, then n_plain riders): a self-attention call (ctx == NULL, ip == NULL) with mode INNER or OUTER; args->coef /
 * begin / end are not read.
 *   OUTER  the workspace has M rows of k / V^T more than n_frames; one AID_KF_GET (aid_keyframe_rows or _q8, M rows) fills rows
 *          n_frames + m from the stores, and the composition of aid_attn_corners_fwd runs with corner rows n_frames + m.
 *   INNER  no extra rows: aid_mix_kv_stores writes the call's k2 / vt2, then the one aid_attn_fwd of the INNER composition runs
 *          (coefficient 0.5 for every AID frame, -1 for the riders: no frame reads an end-point row).
 * The workspace must hold aid_processor_kf_blend_workspace_bytes() bytes (0 for a call that would be refused).  b == NULL is
 * aid_processor_fwd.  ctx != NULL, ip != NULL, mode == PLAIN and every AID_ERR_ARG / AID_ERR_SHAPE of AidKeyframeBlend above are
 * refused with everything aid_processor_fwd checks, before the first launch.  LoRA / DoRA, LayerNorm (folded or not), residual,
 * attn_bias (not with fused), f32_split / f32_attn_split and cu_share work as in aid_processor_fwd: it is the same code path.
 * ------------------------------------------------------------------------------------- */
typedef struct AidKeyframeBlend {
    const AidKeyframeRow* rows;  /* HOST: n_corners entries (k_store, vt_store; `row` ignored) */
    const int32_t*        step;  /* DEVICE                                                     */
    const float*          weights; /* DEVICE fp32 [n_frames, n_corners], as AidCorners.weights */
    int32_t n_corners;           /* 1 .. AID_MAX_CORNERS                                       */
    int32_t n_steps;
    int32_t q8;                  /* 0: native stores, 1: 8-bit block stores                    */
} AidKeyframeBlend;

int    aid_mix_kv_stores(const AidKeyframeBlend* b /* host */, void* k2, void* vt2, int32_t n_frames, int32_t n_plain, int64_t k_fs,
                         int64_t vt_fs, int32_t vt_ld, int32_t vt_cols, int32_t dtype, void* stream);
size_t aid_processor_kf_blend_workspace_bytes(const AidProcessorArgs* args /* host */, const AidKeyframeBlend* b /* host */);
int    aid_processor_kf_blend_fwd(const AidProcessorArgs* args /* host */, const AidKeyframeBlend* b /* host */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Live kernel timing (bench.py's roofline leg): between aid_profile_begin() and
 * aid_profile_end() every kernel launched through this library is bracketed by a pair of
 * HIP events recorded on the launch stream.  aid_profile_end() synchronises those events and
 * returns one entry per launch: elapsed milliseconds plus the ALGORITHMIC work of the launch
 * (flops: 2*m*n*(k + lr_k) per GEMM problem, 4*s*l*c per (frame, key segment) of attention with the
 * segment count of SURVEY.md §8d: plain 1, pure inner 1, fused inner 2, pure outer 2, fused
 * outer 3; bytes: operands read once + result written once).  Not for use inside stream capture.
 * ------------------------------------------------------------------------------------- */
typedef struct AidProfileEntry {
    char   kernel[64];     /* kernel that ran: "aid_attn<f16,d40,inner,nw4>", "aid_gemm_nt_pp_kernel<bf16>", ... */
    double ms;
    double flops;          /* algorithmic                                                      */
    double bytes;
    double flops_executed; /* what the launch really computes: attention with the executed segment count      */
                           /* (AidAttnArgs.seg_executed), GEMM = algorithmic                                  */
} AidProfileEntry;

int aid_profile_begin(void);
/* returns the number of entries written (<= max_entries) or a negative error code */
int aid_profile_end(AidProfileEntry* entries /* host */, int max_entries);

/* misc */
int         aid_abi_version(void);
const char* aid_strerror(int code);
/* name of the kernel variant the last aid_attn_fwd call on this thread launched (for profiling) */
const char* aid_last_attn_variant(void);
/* same for the last aid_gemm_nt launch: "lockstep128", "pingpong256" (+ "+tail128") or "edge"; float32: "f32" (exact) or "f32x3" (split) */
const char* aid_last_gemm_variant(void);
/* Thread safety (ABI v7): every entry point may be called from several host threads at once, each on its own stream with its own
 * workspace.  The tuning table is a set of independent atomic integers (a knob flipped by one thread is seen by the launches of all),
 * the profiling list is guarded by a mutex and collects the launches of every thread between begin and end, the error / variant
 * strings are thread-local. */
/* Development / tuning knobs (kernel-variant choices the launch heuristics normally make: "GEMM_VARIANT", "GEMM_PP",
 * "ATTN_NW", "ATTN_RES", ... — the list is in csrc/aid_kernels.hpp).  The table is filled ONCE when the library is
 * loaded, from environment variables AID_<NAME>; this call changes an entry at run time (value < 0 = back to the
 * heuristic).  Nothing on the launch path reads the environment.  Every value a knob accepts selects among kernels that compute the
 * same result; a value outside a knob's range is refused (AID_ERR_ARG) here and ignored in the environment — no setting can make the
 * library skip work.  Returns AID_ERR_ARG for an unknown name.
 * "CU_SHARE" = n (1 .. 8) is the process-wide default of the per-call hint AidGemmProblem.cu_share / AidProcessorArgs.cu_share (n
 * independent launch streams run side by side; the GEMM engine choice plans with 1 / n of the CUs) for callers that cannot pass it per
 * call; a per-call value > 0 wins.  Results do not depend on it. */
int aid_set_tuning(const char* name, int value);
/* current value of a knob (-1 = the launch heuristics decide) */
int aid_get_tuning(const char* name, int* value);
/* device properties of the current device: returns AID_OK and fills what is non-NULL */
int aid_device_info(int* n_cu, int* clock_khz, char* arch /* >= 32 bytes */);
/* ABI v7.  *id = the id of the stream capture `stream` is part of (hipStreamGetCaptureInfo), 0 when it is not capturing.  Callers that
 * own scratch memory use it to give every capture its own (the Python layer never allocates a workspace inside a capture). */
int aid_stream_capture_id(void* stream, unsigned long long* id);

#ifdef __cplusplus
}
#endif
#endif /* AID_HIP_H */
