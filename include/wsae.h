/*
 * wsae.h -- C ABI of libwsae_hip.so: the MI355X (gfx950 / CDNA4) SAE train-step kernels.
 *
 * This is the drop-in boundary underneath the reference's Python module API.  The reference
 * (omarkhursheed/whisper-sae) has no FFI layer of its own: its hot path is an implicit ATen op
 * sequence issued from src/whisper_sae/sae/model.py and src/whisper_sae/sae/training.py.  Each
 * entry point below names the reference lines whose arithmetic it replaces; the ctypes binding a
 * maintainer adds on the reference side is shown in INTEGRATION.md and lives, for this build, in
 * whisper-sae_amd/whisper_sae/_native.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every data pointer is a caller-owned DEVICE pointer (e.g. torch.Tensor.data_ptr()); nothing
 *     is retained past the call except what a wsae_ctx / wsae_ring handle allocates for itself.
 *   - every launch goes to the caller's stream (hipStream_t passed as void*); no hidden
 *     synchronisation, no allocation inside launch functions (graph-capturable).
 *   - return value: 0 = ok, negative = error; wsae_last_error() gives the thread-local message.
 *   - one ctx per device per process; a ctx is not thread-safe.
 *
 * Flat parameter layout ("pack"): all five parameter tensors of a TopKSAE live in ONE float32
 * buffer of wsae_param_count(D,H) elements (gradients, Adam exp_avg and exp_avg_sq use the same
 * layout in their own buffers), so the optimizer is one pass and the data-parallel exchange is one
 * RCCL all-reduce:
 *     [ W_e  : H*D ]  encoder.weight, row-major [H][D]            (model.py:63)
 *     [ W_dT : H*D ]  decoder.weight TRANSPOSED, row-major [H][D] (model.py:64; row h = decoder
 *                     column h, so decode gathers contiguous rows and the unit-norm constraint of
 *                     model.py:91-96 is a per-row operation)
 *     [ b_e  : H   ]  encoder.bias
 *     [ b_d  : D   ]  decoder.bias
 *     [ b_pre: D   ]  pre-encoder bias                            (model.py:67)
 */
#ifndef WSAE_H_
#define WSAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSAE_VERSION 1

/* error codes */
#define WSAE_OK 0
#define WSAE_ERR_INVALID (-1) /* bad argument / unsupported shape */
#define WSAE_ERR_HIP (-2)     /* a HIP runtime call failed */
#define WSAE_ERR_NOMEM (-3)

/* arithmetic mode of the two contractions (encode GEMM, weight-gradient GEMMs) */
#define WSAE_PREC_BF16 0 /* bf16 MFMA operands, fp32 accumulate ("use_amp": training.py:73-75,179) */
#define WSAE_PREC_FP32 1 /* fp32 MFMA (v_mfma_f32_32x32x2_f32), the reference's CPU fp32 semantics */

/* element type of an activation buffer handed in */
#define WSAE_DT_F32 0
#define WSAE_DT_BF16 1

typedef struct wsae_ctx wsae_ctx;
typedef struct wsae_ring wsae_ring;

typedef struct wsae_config {
    int32_t input_dim;  /* D: multiple of 32, <= 2048 */
    int32_t hidden_dim; /* H: multiple of 32 */
    int32_t k;          /* TopK k: 1..128, <= H */
    int32_t max_batch;  /* largest B any call will pass */
    int32_t precision;  /* WSAE_PREC_* */
    int32_t device;     /* HIP device ordinal */
} wsae_config;

/* device-side step record written by the kernels, fetched lazily by the host
 * (replaces the five .item() syncs of training.py:207-213) */
typedef struct wsae_stats {
    float loss;        /* mean((recon-x)^2)                 model.py:145 */
    float l0;          /* mean_b count(hidden>0)            model.py:148 */
    float grad_norm;   /* global L2 norm before clipping    training.py:188 */
    float clip_coef;   /* min(1, max_norm/(norm+1e-6)) */
    float dead_ratio;  /* get_dead_feature_ratio()          model.py:192-195 */
    int32_t dead_count;
    int32_t topk_fallback_rows; /* rows that took the exact bisection path of the TopK kernel */
    int32_t reserved;
} wsae_stats;

const char* wsae_last_error(void);
int wsae_version(void);

/* number of float32 elements of the flat pack, and element offsets of its five segments
 * (order: W_e, W_dT, b_e, b_d, b_pre) */
int64_t wsae_param_count(int32_t input_dim, int32_t hidden_dim);
int wsae_param_offsets(int32_t input_dim, int32_t hidden_dim, int64_t offsets[5]);

/* ctx: dims + mode + all workspace (bf16 weight shadows, TopK scratch, partial-sum slabs). */
int wsae_ctx_create(const wsae_config* cfg, wsae_ctx** out);
int wsae_ctx_destroy(wsae_ctx* ctx);
/* Data-parallel dead-feature clock without a second collective.  `fired` = float[hidden_dim], zero
 * before the first step, or NULL to switch the mechanism off (the default).  When set:
 *   - wsae_decode_loss stores 1.0f to fired[f] for every feature f it stamps in last_activated
 *     (model.py:178-181);
 *   - the caller sums `fired` over the ranks (it rides at the tail of the gradient all-reduce);
 *   - wsae_adamw_step then sets last_activated[f] = *step_count wherever fired[f] > 0 and clears
 *     fired for the next step.
 * With clocks that agreed before the step this equals all_reduce(MAX) of last_activated: a feature
 * either fired somewhere in this step (new value = the step) or nowhere (value unchanged, equal on
 * every rank).  Replaces the 8*H-byte MAX all-reduce the reference's semantics would otherwise need
 * under DDP (the reference itself is single-process). */
int wsae_ctx_set_fired(wsae_ctx* ctx, float* fired);
/* Selective strip stores of the encoder GEMM (no counterpart in the reference: a property of this implementation of
 * model.py:111-114).  The TopK of wsae_encode_topk / wsae_encode_decode reads a 16-column strip of the pre-activation
 * matrix only when the strip's maximum reaches the row's threshold T, so for batches served by the persistent GEMM
 * (bf16 mode, B >= 2048) that GEMM writes to HBM only the strips whose maximum reaches s x the smallest T of the
 * previous TWO batches on this ctx, with a margin s that adapts by itself (0.25 .. 1; wsae_topk.h).  The prediction is
 * verified row by row in the TopK launch, and a row that needs a strip that was not stored recomputes it with the GEMM's
 * own arithmetic: outputs are bit-identical with the feature on or off, whatever the history; only the time differs
 * (DESIGN.md section 4.1).
 *   on: 0 disables, non-zero enables (default: enabled, or disabled when the environment has WSAE_STRIP_PREDICT=0 at
 *   wsae_ctx_create time - for A/B timing runs; WSAE_STRIP_SAFETY=<s> there fixes the margin).
 *   assume_store_threshold: NaN forgets the history (the next launch stores every strip); any other value is the store
 *   threshold the next launch uses (tests pass a huge value to force every row through the recompute path). */
int wsae_ctx_set_strip_predict(wsae_ctx* ctx, int32_t on, float assume_store_threshold);
/* refilled_rows: rows that recomputed strips since the ctx was created (cumulative); last_min_threshold: the smallest row
 * threshold of the last predicated TopK launch (NaN when there is none); margin: the s of the last predicated GEMM launch
 * (0 when there is none).  Synchronises the device. */
int wsae_ctx_strip_stats(wsae_ctx* ctx, int64_t* refilled_rows, float* last_min_threshold, float* margin);
/* Number of columns the reconstruction MSE (and g = 2 r / (B cols)) averages over; default input_dim.  A transcoder
 * whose output is narrower than its input runs on a ctx padded to the wider of the two and sets this to its
 * output_dim (F.mse_loss means over B * output_dim, transcoder.py:152). */
int wsae_ctx_set_loss_cols(wsae_ctx* ctx, int32_t cols);
size_t wsae_ctx_workspace_bytes(const wsae_ctx* ctx);
/* Allocate the dense workspace of the ReLU SAE path (3 x max_batch x hidden_dim operand copies) on the ctx's
 * device.  Call once after wsae_ctx_create, before the first wsae_relu_forward: launch functions never allocate. */
int wsae_ctx_reserve_relu(wsae_ctx* ctx);

/* Refresh what the kernels derive from the master weights: bf16 shadow of W_e and the folded
 * encoder bias c[h] = b_e[h] - bf16(W_e)[h,:] . b_pre (BF16 mode).  Must be called after any
 * change to `params` that did not go through wsae_adamw_step (which refreshes them itself). */
int wsae_prepare(wsae_ctx* ctx, const float* params, void* stream);

/* ---- forward --------------------------------------------------------------------------------
 * x: [B, D] activations of dtype x_dtype; `rows` (nullable) gathers: batch row b is x[rows[b], :]
 * (this is how batches are drawn from the on-device ring buffer without a copy). */

/* TopKSAE.encode up to the TopK (model.py:108-114): pre = (x - b_pre) W_e^T + b_e, then the k
 * largest per row, sorted descending (ties: lowest index first).  Compact code out:
 * vals [B,k] f32 (pre-activation values, NOT yet relu'd), idx [B,k] i32.
 * step_count (nullable, device int64): incremented by one = the dead-feature clock of
 * model.py:175; pass it only for training-mode forwards. */
int wsae_encode_topk(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                     const int32_t* rows, int32_t B, float* vals, int32_t* idx,
                     int64_t* step_count, wsae_stats* stats, void* stream);

/* Dense pre-activations [B,H] f32 (model.py:111), for API users / tests. */
int wsae_encode_dense(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                      const int32_t* rows, int32_t B, float* pre, void* stream);

/* hidden = zeros; hidden[idx] = relu(vals) (model.py:115-116).  hidden: [B,H] f32. */
int wsae_densify(wsae_ctx* ctx, const float* vals, const int32_t* idx, int32_t B, float* hidden,
                 void* stream);

/* TopKSAE.decode for an arbitrary dense code (model.py:129): recon = hidden W_d^T + b_d + b_pre. */
int wsae_decode_dense(wsae_ctx* ctx, const float* params, const float* hidden, int32_t B,
                      float* recon, void* stream);

/* Sparse decode + MSE + (optionally) the first half of backward, one pass over the compact code
 * (model.py:129,145,148,168-181 and the autograd of them):
 *   recon = sum_j relu(v_j) W_dT[idx_j,:] + b_d + b_pre ; loss = mean((recon-x)^2) ; l0
 *   want_bwd bit 0: g = 2 (recon-x)/(B*D) kept in ctx workspace (in the contraction dtype),
 *            dpre[b,j] = (v_j>0) ? g . W_dT[idx_j,:] : 0;   bit 1 (value 2, with bit 0): also keep the fp32 g that
 *            wsae_input_grad reads (only the autograd API path needs dL/dx)
 *   last_activated (nullable, device int64[H]) with step_count (device int64): features with
 *   v_j > 0 get last_activated = *step_count.
 * recon (nullable): [B,D] f32.  dpre (required when want_bwd): [B,k] f32.
 * stats->loss / stats->l0 are written (device). */
int wsae_decode_loss(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                     const int32_t* rows, const float* vals, const int32_t* idx, int32_t B,
                     float* recon, int32_t want_bwd, float* dpre, int64_t* last_activated,
                     const int64_t* step_count, wsae_stats* stats, void* stream);

/* TopKSAE.forward in one call (model.py:131-166) = wsae_encode_topk followed by wsae_decode_loss on the same batch:
 * same arguments, same outputs (vals / idx are OUTPUTS here), same record. */
int wsae_encode_decode(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype, const int32_t* rows,
                       int32_t B, float* vals, int32_t* idx, int64_t* step_count, float* recon, int32_t want_bwd,
                       float* dpre, int64_t* last_activated, wsae_stats* stats, void* stream);

/* Second half of backward (autograd of model.py:111,129 w.r.t. the parameters): the two
 * [H,B]x[B,D] contractions on MFMA with the sparse operand rebuilt in LDS from the compact code,
 * plus the three bias gradients.  Needs the g left in ctx by wsae_decode_loss(want_bwd=1) on the
 * same batch, and the SAME x / x_dtype / rows as that forward (a bf16 batch in BF16 mode is not staged by the
 * forward: this call transposes it for the dW_e contraction).  grads: flat pack, overwritten.
 * In BF16 mode with input_dim > 256 behind the MFMA decode launch the code is contracted on the 2:4 sparse MFMA
 * (v_smfmac_f32_32x32x32_bf16: exact for every code, deterministic).  WSAE_WGRAD_SPARSE=0 in the
 * environment at wsae_ctx_create time keeps the dense form (A/B runs and tests); the two differ in the last bits. */
int wsae_weight_grads(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                      const int32_t* rows, const float* vals, const int32_t* idx,
                      const float* dpre, int32_t B, float* grads, void* stream);

/* ---- BatchTopK (Bussmann, Leask & Nanda 2024) ------------------------------------------------
 * Over the compact code of the per-row TopK (vals [B, k] with k = the ctx's k, here the per-row cap k_max; each row sorted
 * descending): t = the (B k_batch)-th largest POSITIVE value of the batch (the smallest positive one when there are fewer);
 * a candidate is kept iff v > 0 and v >= t (ties at t all kept), every other one is overwritten with 0.0f (its index is
 * left in place).  Decode, backward, l0 and the dead-feature clock treat v <= 0 as inactive, so the masked code feeds
 * them unchanged.  Modes:
 *   WSAE_BTK_TRAIN   select as above and update the threshold: theta <- t while theta < 0, else
 *                    theta <- beta theta + (1 - beta) t (no update when nothing was kept);
 *   WSAE_BTK_EVAL    keep iff v > 0 and v > theta; while theta < 0 (never trained) select as above, without update;
 *   WSAE_BTK_SELECT  select as above without touching theta (training-mode encode, resampling forwards).
 * The state record is caller-owned device memory; everything runs on the stream, with no host sync. */
#define WSAE_BTK_TRAIN 0
#define WSAE_BTK_EVAL 1
#define WSAE_BTK_SELECT 2
typedef struct wsae_batch_topk_state {
    float threshold;        /* theta, -1 = never trained (set by the caller at creation) */
    float beta;             /* EMA factor of theta (set by the caller) */
    float last_t;           /* t of the last selection (theta in threshold mode), -1 when no candidate was positive */
    int32_t saturated_rows; /* rows whose k_max-th candidate was kept (0 when k_max = hidden_dim) */
    int32_t kept;           /* entries kept by the last selection */
    int32_t reserved[3];
} wsae_batch_topk_state;
/* The selection alone, in place on vals [B, ctx k] (16-byte aligned); 1 <= k_batch <= ctx k. */
int wsae_batch_topk_select(wsae_ctx* ctx, float* vals, int32_t B, int32_t k_batch, int32_t mode,
                           wsae_batch_topk_state* state, void* stream);
/* Run the selection inside wsae_encode_topk and wsae_encode_decode, between the TopK and the decode (k_batch = 0, the
 * default: off - no extra launch, outputs bit-identical to a ctx that never heard of it).  `state` must outlive the calls. */
int wsae_ctx_set_batch_topk(wsae_ctx* ctx, int32_t k_batch, int32_t mode, wsae_batch_topk_state* state);

/* ---- data parallel: the gradients go straight onto the exchange buffer -------------------------------------------
 * (absent from the reference, which is single-process).  The WIRE is what the ranks
 * all-reduce(SUM): `hidden_dim * input_dim` elements of dW_dT, then dW_e, db_e, db_d, db_pre (the rest of the pack) and
 * the `hidden_dim` fired indicators of wsae_ctx_set_fired, then WSAE_WIRE_METRIC_SLOTS metric digits (below): P + hidden_dim +
 * WSAE_WIRE_METRIC_SLOTS elements of `wire_dtype` (WSAE_DT_F32: the exact data-parallel gradient; WSAE_DT_BF16: half the bytes
 * over xGMI, every rank's gradient rounded once to bf16, the indicators - sums of at most world_size ones - and the digits
 * exact).  Normally ONE call with part = WSAE_PART_ALL and one all-reduce.  The decoder matrix comes FIRST so that the
 * optional two halves of the backward fill two contiguous ranges:
 *   part = WSAE_PART_DECODER  contraction of dW_dT alone (split-K 16) + its reduction -> wire[0, H D)
 *   part = WSAE_PART_ENCODER  contraction of dW_e alone + reduction + the three bias gradients + the indicators
 *                             -> wire[H D, P + H)          (same batch, after the decoder part)
 *   part = WSAE_PART_ALL      both contractions in one launch (the single-GPU geometry) -> the whole wire
 * With halves the caller starts the all-reduce of wire[0, H D) after the decoder part, on its communication stream, and it runs
 * under the encoder part's contraction (measured on MI355X: the split costs +86 us of kernels and stream hand-overs per step
 * against +16 us for WSAE_PART_ALL with one in-stream collective - DESIGN.md section 6).  Halves need input_dim > 256 (wsae_wgrad_parts_supported); the gradient pack in
 * `grads` form is NOT written by these calls: wsae_grads_unpack_wire produces it from the summed wire. */
#define WSAE_PART_ALL (-1)
#define WSAE_PART_DECODER 0
#define WSAE_PART_ENCODER 1
int wsae_wgrad_parts_supported(const wsae_ctx* ctx);
/* Compute units the ENCODER part leaves without a workgroup (default 0).  The contraction's workgroups fill the register
 * file of the CU they sit on (two waves x ~246 VGPRs per SIMD), so the collective of the decoder half, issued on another
 * stream while the encoder part runs, only overlaps if some CUs are free for its kernels; the part then runs split-K 13
 * or 14 instead of 16 (a few percent longer).  Unmeasured on hardware so far: the builder's boxes have one GPU. */
int wsae_ctx_set_comm_reserve(wsae_ctx* ctx, int32_t n_cus);
int wsae_weight_grads_wire(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                           const int32_t* rows, const float* vals, const int32_t* idx, const float* dpre,
                           int32_t B, int32_t part, void* wire, int32_t wire_dtype, void* stream);

/* Copy of g = 2 (recon - x) / (B cols), fp32 [B, D], as left by the last wsae_decode_loss with want_bwd = 3: the
 * gradient of the loss w.r.t. the reconstruction (= minus its gradient w.r.t. the target; transcoder skip path). */
int wsae_last_residual_grad(wsae_ctx* ctx, int32_t B, float* g_out, void* stream);

/* dL/dx (only the autograd API path needs it): dx = dpre W_e - g (subtract_g = 1: the SAE, whose target is its
 * input; needs the fp32 g, want_bwd = 3) or dx = dpre W_e (subtract_g = 0: transcoders).  dx: [B,D] f32. */
int wsae_input_grad(wsae_ctx* ctx, const float* params, const int32_t* idx, const float* dpre,
                    int32_t B, float* dx, int32_t subtract_g, void* stream);

/* ---- optimizer tail (training.py:186-198, :212) -------------------------------------------------
 * global-L2 clip (clip_grad_norm_, max_norm <= 0 disables) -> AdamW (torch semantics, step is the
 * 1-based update count) -> decoder column renorm (model.py:91-96, if normalize_decoder) ->
 * refresh of the derived shadows -> optional dead-feature scan (model.py:183-195) into stats.
 * grads are scaled by grad_scale first (1/world_size after a SUM all-reduce).
 * norm_from_wgrad: 1 = `grads` is exactly what the preceding wsae_weight_grads on this ctx wrote
 *   (single GPU): the global norm comes from the partial sums that call left behind and one pass
 *   over the gradients is saved; 0 = the gradients were touched since (all-reduce): recompute; 2 = use the partial sums
 *   if the preceding backward on this ctx left any (wsae_relu_backward does on its row-major-GEMM flow), else recompute.
 * last_activated (nullable) / step_count / dead_threshold: when given, stats->dead_count and
 *   stats->dead_ratio are written (get_dead_feature_ratio() of training.py:212).
 * All four buffers use the flat pack layout.
 * lr, beta1, beta2, eps, weight_decay are doubles, as torch holds them: 1 - beta1, 1 - beta2, 1 - lr * weight_decay and the
 * bias corrections are formed in double and rounded once to fp32, so exp_avg / exp_avg_sq carry torch.optim.AdamW's own
 * constants (float32(1 - beta), not 1 - float32(beta), which is 1.29e-5 away for beta2 = 0.999). */
/* Data parallel: turn the SUMMED wire (layout above, P + hidden_dim elements of wire_dtype) into the fp32 buffer
 * `grads_ext` = [gradient pack in pack order | fired] that wsae_adamw_step reads, and leave the gradient part's
 * squared-norm partials in the ctx, so that the following wsae_adamw_step(norm_from_wgrad = 1, grad_scale = 1 / world)
 * needs no norm pass of its own.  metrics_sum: float[2] = the ranks' summed (loss, l0) of this step from an exchange of the
 * caller's own (may be the loss / l0 words of `stats` themselves), or NULL = take them from the wire's metric elements (when
 * wsae_ctx_set_wire_metrics named a source for them); stats->loss / stats->l0 are overwritten with their means over `world`
 * ranks. */
/* The step's two metric scalars ride on the wire as well (a separate 8-byte all-reduce costs a data-parallel step 16 us of
 * stream hand-over on MI355X): behind the fired indicators the wire carries WSAE_WIRE_METRIC_SLOTS more elements, written by
 * the reduction launch that writes the indicators from the two floats at `loss_l0` (device memory, e.g. the first two words
 * of the step's wsae_stats record; NULL = zeros) - the loss as 40-bit fixed point (2^-24 resolution, range 65536) in ten
 * base-16 digits, l0 as 32-bit fixed point (2^-16) in eight, one digit per element, a non-finite flag in the element after:
 * digit sums over up to 16 ranks stay below 256 and are therefore EXACT in a bf16 all-reduce as well.
 * wsae_grads_unpack_wire(metrics_sum = NULL) decodes them and writes the rank means into stats.  The wire is thus
 * P + hidden_dim + WSAE_WIRE_METRIC_SLOTS elements long. */
#define WSAE_WIRE_METRIC_SLOTS 24
int wsae_ctx_set_wire_metrics(wsae_ctx* ctx, const float* loss_l0);
int wsae_grads_unpack_wire(wsae_ctx* ctx, const void* wire, int32_t wire_dtype, float* grads_ext,
                           const float* metrics_sum, int32_t world, wsae_stats* stats, void* stream);
int wsae_adamw_step(wsae_ctx* ctx, float* params, const float* grads, float* exp_avg,
                    float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int32_t step, float max_norm, float grad_scale,
                    int32_t normalize_decoder, int32_t norm_from_wgrad,
                    int64_t* last_activated, const int64_t* step_count,
                    int64_t dead_threshold, wsae_stats* stats, void* stream);

/* F.normalize(decoder.weight, dim=0) alone (model.py:91-96) + shadow refresh. */
int wsae_normalize_decoder(wsae_ctx* ctx, float* params, void* stream);

/* ---- dead features (model.py:183-257) -------------------------------------------------------- */
/* stats->dead_count / dead_ratio = #(step_count - last_activated > threshold); mask (nullable):
 * uint8[H]. */
int wsae_dead_scan(wsae_ctx* ctx, const int64_t* last_activated, const int64_t* step_count,
                   int64_t threshold, uint8_t* mask, wsae_stats* stats, void* stream);

/* resample_dead_features (model.py:197-257).  Call order mirrors the reference: (1) wsae_dead_scan
 * -> dead_mask (model.py:215, BEFORE the forward); (2) the forward on `inputs` (encode_topk +
 * decode_loss with a recon buffer; in train mode it bumps the dead-feature clock, model.py:229);
 * (3) wsae_row_errors -> row_err [Br] = sum_d (x-recon)^2; (4) wsae_resample_dead: dead features
 * ascending (at most num_cap, <0 = all), rows by error descending, the L2-normalised raw input row
 * goes to W_e[f,:] and W_dT[f,:], b_e[f] = 0, last_activated[f] = *step_count.  Adam moments
 * untouched.  n_dead_out (device int32): the capped dead count the reference returns
 * (model.py:257), even when fewer than that many rows exist.  Br <= min(max_batch, 16384): the row sort holds one 64-bit
 * key per row, rounded up to a power of two, in LDS (128 KB at 16384 rows; wsae_ctx_create raises the kernel's
 * dynamic-LDS limit for it, and a device that grants a block less than 128 KB is held to 8192 rows). */
/* Transcoders (sae/transcoder.py:207-252): wsae_row_errors takes the TARGET as x and may also leave the residual
 * rows resid [Br, D] = x - recon (nullable); wsae_resample_dead then writes the L2-normalised row of dec_src
 * (nullable: the residuals) into the decoder column instead of the input direction. */
int wsae_row_errors(wsae_ctx* ctx, const void* x, int32_t x_dtype, const int32_t* rows,
                    const float* recon, int32_t B, float* row_err, float* resid, void* stream);
int wsae_resample_dead(wsae_ctx* ctx, float* params, const void* inputs, int32_t x_dtype,
                       const int32_t* rows, int32_t Br, const float* row_err,
                       const uint8_t* dead_mask, int64_t* last_activated,
                       const int64_t* step_count, int32_t num_cap, int32_t* n_dead_out,
                       const float* dec_src, void* stream);

/* ---- on-device activation ring buffer (replaces data/feature_cache.py:169-197) ---------------
 * capacity rows of D elements (bf16 or f32) resident in HBM; producers push blocks of rows,
 * the trainer draws batches as row-index lists (a seeded permutation per epoch), and the kernels
 * gather rows straight from the ring. */
int wsae_ring_create(int32_t device, int64_t capacity_rows, int32_t dim, int32_t dtype,
                     wsae_ring** out);
int wsae_ring_destroy(wsae_ring* ring);
/* Producer side (row N2, sae/hooks.py:86-92): rows of hidden states [n_rows, dim] go through LayerNorm(gamma, beta, eps;
 * biased variance, as torch.nn.LayerNorm - Whisper's final encoder / decoder norm) and into the ring in its dtype,
 * one pass, nothing on the host. */
int wsae_ring_push_layernorm(wsae_ring* ring, const void* src, int32_t src_dtype, int64_t n_rows,
                             const float* gamma, const float* beta, float eps, void* stream);
void* wsae_ring_data(wsae_ring* ring);         /* device pointer of row 0 */
int64_t wsae_ring_size(const wsae_ring* ring); /* rows currently valid */
/* append n_rows rows ([n_rows, D], device pointer, src_dtype f32/bf16 -> converted to the ring's
 * dtype), wrapping around and overwriting the oldest rows once full */
int wsae_ring_push(wsae_ring* ring, const void* src, int32_t src_dtype, int64_t n_rows, void* stream);
/* rows_out[i] = perm_{seed,epoch}(offset + i) mod size, i < n: a bijective shuffle of [0,size)
 * (the RandomSampler of feature_cache.py:191-197), computed on device */
int wsae_ring_sample(wsae_ring* ring, uint64_t seed, int64_t epoch, int64_t offset, int32_t n,
                     int32_t* rows_out, void* stream);
/* fill with deterministic synthetic activations ~N(0,1) (bench / tests) */
int wsae_ring_fill_synthetic(wsae_ring* ring, uint64_t seed, int64_t n_rows, void* stream);

/* ---- causal feature interventions (row N5) ------------------------------------------------
 * The consumer on the other side of the hooks: a block's output h [n_rows, dim] goes through the component's final
 * LayerNorm (wsae_layernorm_rows: the row LayerNorm of wsae_ring_push_layernorm to a plain buffer dst [n_rows, dim] of
 * dst_dtype), the SAE's compact code of it is edited, and the edit is written back into h in the model's own
 * coordinates (wsae_intervene).  Per row, with mu and sigma = sqrt(var + eps) of h frozen, a = LN(h), (v_j, i_j) the
 * row's code, act_j = max(v_j, 0):
 *   act'_j = scale[i_j] * act_j, or c_f where i_j is a forced feature f; rows with row_mask[r] == 0 keep act'_j = act_j
 *            and take no forced term (row_mask NULL = every row; scale NULL = all ones);
 *   WSAE_IV_KEEP_ERROR  h' = h + sigma * (sum_j (act'_j - act_j) W_dT[i_j,:] + sum_{forced f not in the code} c_f W_dT[f,:]) / gamma
 *   WSAE_IV_REPLACE     h' = mu + sigma * (b_d + b_pre + sum_j act'_j W_dT[i_j,:] + the same forced terms - beta) / gamma
 * gamma == NULL: no norm (a = h, h' = h + delta or the edited reconstruction itself).  Terms with a zero weight are
 * skipped; the others accumulate in fp32 in ascending j, forced terms after them in list order, over the decoder rows
 * the ctx's decode reads (fp32 pack rows in FP32 mode, the bf16 shadow in BF16 mode: wsae_prepare first) - a fixed
 * order, two runs are bit-identical.  A KEEP_ERROR row without a non-zero term is not stored (out == h) or copied
 * (out != h): the identity edit leaves h bit-identical.  vals / idx: [n_rows, ctx k] as wsae_encode_topk wrote them;
 * n_force <= WSAE_IV_MAX_FORCE; out may equal h (then out_dtype == h_dtype); changed_rows (nullable, device int32)
 * receives the number of rows written with an edit (every row in REPLACE mode). */
#define WSAE_IV_KEEP_ERROR 0
#define WSAE_IV_REPLACE 1
#define WSAE_IV_MAX_FORCE 64
int wsae_layernorm_rows(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, const float* gamma,
                        const float* beta, float eps, void* dst, int32_t dst_dtype, void* stream);
int wsae_intervene(wsae_ctx* ctx, const float* params, const void* h, int32_t h_dtype, int64_t n_rows,
                   const float* vals, const int32_t* idx, const float* gamma, const float* beta, float eps,
                   const float* scale, const int32_t* force_idx, const float* force_val, int32_t n_force,
                   const uint8_t* row_mask, int32_t mode, void* out, int32_t out_dtype, int32_t* changed_rows,
                   void* stream);

/* ---- feature attribution (attribution patching) ---------------------------------------------
 * The first-order effect on a scalar metric m of the edit wsae_intervene applies in WSAE_IV_KEEP_ERROR mode, for every
 * code entry and per feature, from one gradient: grad_h = G = dm/dh' [n_rows, dim] with respect to the tapped block's
 * output on the clean run.  Same setting as wsae_intervene: h [n_rows, dim], (gamma, eps) of the component's final
 * LayerNorm, (v_j, i_j) the row's code of a = LN(h).  Since h' = h + sigma (sum_j (act'_j - act_j) W_dT[i_j,:]) / gamma
 * with mu and sigma frozen, per row r and code entry j:
 *   act_j   = max(v_j, 0)
 *   w_j     = (scale[i_j] - 1) * act_j   (scale NULL: ablate everything, w_j = -act_j; rows with row_mask[r] == 0 and
 *                                         entries whose index is outside [0, hidden_dim): w_j = 0)
 *   s_j     = sum_d (G[r,d] / gamma_d) * W_dT[i_j, d]          (gamma NULL: G[r,d] itself, and sigma = 1)
 *   attr_rj = sigma_r * w_j * s_j,       sigma_r = sqrt(var_r + eps), biased variance (the statistics of wsae_intervene)
 * This is the exact first-order term of the intervention, which freezes each row's statistics; it is not the derivative
 * through a differentiated LayerNorm.  Forced (clamped) features and WSAE_IV_REPLACE are out of scope.  W_dT: the
 * decoder rows the ctx's decode reads (fp32 pack rows in FP32 mode, the bf16 shadow in BF16 mode: wsae_prepare first).
 * u_d = G_d / gamma_d is rounded once, s_j accumulates in fp32 (fmaf), attr = (sigma * w_j) * s_j.  An entry with
 * w_j == 0 gets attr_rj = 0.0f exactly and its decoder row is not read.
 * Inputs are expected to be finite.  A non-finite attr_rj anywhere in the call (an Inf or NaN gradient, an overflow) is
 * propagated, not hidden: attr carries it, feat_sum and feat_abs are NaN for every feature, feat_rows stays exact.
 * Per feature f over the whole call (each output nullable; any of them needs the workspace):
 *   feat_sum[f] = sum of attr_rj over the entries with i_j == f, feat_abs[f] the same over |attr_rj|,
 *   feat_rows[f] = number of entries with i_j == f and w_j != 0.
 * The sums are exact fixed point: A = max |attr_rj| of the call, A < 2^e, q = 2^(e - 36); every entry adds the integer
 * rint(attr_rj / q) to a 64-bit accumulator and the result is float(acc * q), rounded once (error <= q / 2 per entry
 * plus that rounding; A == 0: zeros).  n_rows * k <= 2^26, so the accumulators cannot overflow.  No float atomics: two
 * calls give the same bits, attr of a row depends on that row alone, and feat_sum / feat_abs depend neither on the
 * launch geometry nor on the order of the rows.  h, grad_h: f32 or bf16; vals / idx / attr: [n_rows, ctx k];
 * workspace: wsae_attribute_workspace_bytes(hidden_dim) bytes, 8-byte aligned, cleared inside the call. */
int64_t wsae_attribute_workspace_bytes(int32_t hidden_dim);
int wsae_attribute(wsae_ctx* ctx, const float* params, const void* h, int32_t h_dtype, const void* grad_h,
                   int32_t grad_dtype, int64_t n_rows, const float* vals, const int32_t* idx, const float* gamma,
                   float eps, const float* scale, const uint8_t* row_mask, float* attr, float* feat_sum, float* feat_abs,
                   int32_t* feat_rows, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- in-library kernel timing (bench.py's roofline leg) ----------------------------------------
 * When enabled for a kernel id, every launch of that kernel on this ctx is bracketed by a pair of
 * HIP events recorded on the launch stream (up to max_samples launches, then recording stops).
 * wsae_profile_read synchronises the recorded events and returns launch count and summed
 * duration.  kernel_id -1 = all kernels.  Ids: see wsae_kernel_name(). */
#define WSAE_K_STAGE_BATCH 0
#define WSAE_K_ENCODE_GEMM 1
#define WSAE_K_TOPK 2          /* standalone TopK launch (absent from the fused training forward) */
#define WSAE_K_DECODE 3        /* decode + loss + dpre (+ the fused TopK) */
#define WSAE_K_BUCKET 4        /* counting sort of the compact code + g transposition */
#define WSAE_K_WGRAD 5         /* the two weight-gradient contractions */
#define WSAE_K_WGRAD_REDUCE 6  /* split-K reduction + bias gradients */
#define WSAE_K_SQNORM 7
#define WSAE_K_ADAMW 8         /* fused optimizer tail */
#define WSAE_K_ROWNORM 9
#define WSAE_K_PREPARE 10
#define WSAE_K_DEAD_SCAN 11
#define WSAE_K_COUNT 12
const char* wsae_kernel_name(int32_t kernel_id);
int wsae_profile_enable(wsae_ctx* ctx, int32_t kernel_id, int32_t max_samples);
int wsae_profile_disable(wsae_ctx* ctx);
int wsae_profile_read(wsae_ctx* ctx, int32_t kernel_id, int32_t* n_launches, double* total_ms);

/* ---- per-feature top activations (row N4: analysis/feature_viz.py:94-158, TopKTracker.update) -----------------
 * The consumer right after the path: for every feature keep the `keep` (<= 64) strongest positive activations seen
 * so far.  One call = one batch of `rows` activation rows, given either as the compact code the TopK kernel emits
 * (vals/idx [rows][width], width = k) or as a dense matrix (idx == NULL, vals [rows][H], width == H).  Row r of the
 * call is activation number ord_base + r; the caller maps ordinals to (sample, position).  State (caller-owned,
 * zero-initialised, device memory on the current device): top_vals [H][keep] f32 and top_ord [H][keep] i64, both
 * sorted (value descending, then ordinal ascending: the reference keeps the earlier of two equal values,
 * feature_viz.py:153), top_cnt [H] i32, total_active [1] i64 (+= number of entries > 0, feature_viz.py:136).
 * workspace: wsae_feature_topk_workspace_bytes(rows * width, H) bytes of scratch. */
int64_t wsae_feature_topk_workspace_bytes(int64_t max_entries, int32_t H);
int wsae_feature_topk_update(const float* vals, const int32_t* idx, int64_t rows, int32_t width, int32_t H,
                             int32_t keep, int64_t ord_base, float* top_vals, int64_t* top_ord,
                             int32_t* top_cnt, int64_t* total_active, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ---- ReLU SAE (model.py:260-322), dense path ------------------------------------------------- */
/* ReLUSAE has no pre-bias: pass the TopK pack [W_e | W_dT | b_e | b_d | b_pre] with b_pre = 0 (wsae_prepare
 * first, as for the TopK path).  forward:  hidden [B,H] f32 = relu(x W_e^T + b_e) (model.py:307),
 * recon [B,D] f32 = hidden W_d^T + b_d (:308), stats->loss = mse + sparsity_weight * mean|hidden| (:309-311),
 * stats->l0 (:313), stats->reserved = the float bits of mean|hidden|; *sparsity_loss_out likewise (may be
 * NULL, as may stats).  backward (must follow the forward of the same batch on the same ctx: it reuses the
 * staged x^T and hidden^T): grads in pack layout, dW_e, dW_dT, db_e, db_d as autograd of model.py:304-311
 * gives them, the b_pre slot set to 0; no dL/dx (the reference has none either).  Needs wsae_ctx_reserve_relu. */
/* configs[4] of BASELINE.json ("fp8 MFMA encode/decode"): on != 0 makes the two forward GEMMs of wsae_relu_forward take
 * OCP e4m3 copies of their operands (x and hidden quantised per batch row, W_e per feature row, W_d per output row;
 * q = e4m3(v * 448 / amax_row), v_mfma_f32_32x32x16_fp8_fp8, fp32 accumulate, dequantised in the GEMM epilogue).  BF16
 * mode only; hidden, loss and the whole backward stay on the bf16 path.  Needs batch >= 512, input_dim % 256 == 0,
 * hidden_dim % 256 == 0. */
int wsae_ctx_set_relu_fp8(wsae_ctx* ctx, int32_t on);
/* 1 when wsae_relu_forward / wsae_relu_backward at batch size B read / write the dense fp32 `hidden` buffer, 0 when it is
 * optional (bf16 mode, whole 128-row groups, input_dim a multiple of 128, hidden_dim of 256: the hidden code then lives as
 * bf16 in the ctx workspace, written by the encoder GEMM's epilogue, and `hidden` may be NULL - a trainer that never looks at
 * it saves 4 B H bytes of stores per step; a non-NULL `hidden` still receives the fp32 copy).  Where this returns 0, `recon` is
 * optional as well: the forward's residual pass already leaves g = 2 (recon - x) / (B cols) and the db_d partials for the
 * backward of the same batch, which then needs no recon (a non-NULL `recon` still receives the fp32 reconstruction).
 * One exception: wsae_decode_loss / wsae_encode_decode on the same ctx between that forward and its backward take the
 * buffers g and the db_d partials live in (and nothing else the backward reads, as long as the batch is the same); the
 * backward then rebuilds both from `recon`, bit for bit, and returns an error when `recon` is NULL. */
int wsae_relu_needs_hidden(const wsae_ctx* ctx, int32_t B);
/* Per-feature weights w[hidden_dim] of the L1 term (device memory, caller-owned, must outlive the calls; NULL = all ones, the
 * default): the sparsity term of wsae_relu_forward becomes sum_b sum_s w[s] |hidden[b][s]| / (B H) and wsae_relu_backward adds
 * sparsity_weight * w[s] / (B H) to dL/dhidden[b][s] (w itself is a constant of the step).  The cross-layer crosscoder
 * (crosscoder.py:213-217: decoder-norm-weighted L1, mean over the batch of the row sums) passes the decoder norms and
 * sparsity_weight * H.  The MSE of the ReLU path divides by B * loss_cols (wsae_ctx_set_loss_cols), as the TopK path does. */
int wsae_ctx_set_relu_l1_weights(wsae_ctx* ctx, const float* weights);
int wsae_relu_forward(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                      const int32_t* rows, int32_t B, float sparsity_weight, float* hidden,
                      float* recon, wsae_stats* stats, float* sparsity_loss_out, void* stream);
int wsae_relu_backward(wsae_ctx* ctx, const float* params, const void* x, int32_t x_dtype,
                       const int32_t* rows, int32_t B, float sparsity_weight, const float* hidden,
                       const float* recon, float* grads, void* stream);

/* ---- dictionary comparison: nearest rows of B for every row of A ---------------------------
 * For every row i of A [rows_a, dim] the top_n most similar rows j of B [rows_b, dim], without the [rows_a, rows_b]
 * similarity matrix ever existing in memory: a GEMM whose epilogue is the selection.  Ctx-free (two dictionaries of
 * different hidden_dim cannot share a ctx).  A, B: fp32, row-major, leading dimensions lda, ldb >= dim in elements
 * (multiples of 4; the pointers 16-byte aligned), so the W_e or W_dT rows of a pack, or one layer's column slice of a
 * crosscoder's decoder rows, are passed in place.  dim: a multiple of 32, <= 2048.  rows_a, rows_b >= 1, any value;
 * a column >= rows_b is never selected.  1 <= top_n <= WSAE_MATCH_MAX_N.  B may be A.
 * Arithmetic.  WSAE_MATCH_COSINE: a^ = a * (1 / max(sqrt(sum_d a_d^2), 1e-12)), sum and scaling in fp32 (a zero row has
 * similarity 0 to everything), b^ likewise, sim_ij = sum_d a^_id b^_jd.  WSAE_MATCH_DOT: the raw rows.
 * WSAE_PREC_FP32: fp32 MFMA on the fp32 operands.  WSAE_PREC_BF16: the (normalised) operands are rounded once to bf16
 * (nearest even), fp32 accumulate.  A first pass stages the normalised / converted operands in the workspace; the
 * contraction reads the staged copies.  sim_ij depends on row i of A and row j of B alone: every pair is summed in the
 * same K order (ascending K steps of the MFMA, dim rounded up with zeros in BF16 mode), whatever tile, column split or
 * neighbours it has; two calls give the same bits.
 * Selection.  Per row of A the top_n largest sim_ij, sorted by value descending, then index ascending (ties go to the
 * lowest index); this order is total, so the result does not depend on the launch geometry.  exclude_self != 0 skips
 * column j == i (B is A).  With fewer than top_n candidates the tail is idx = -1, val = -inf.  Inputs are expected to
 * be finite.  No float atomics; the column splits hand their candidates to a merge launch through the workspace.
 * workspace: wsae_match_workspace_bytes (-1 for invalid arguments) bytes of device scratch, 16-byte aligned: the two
 * staged operands (rows rounded up to 128) and top_n (rounded up to 4, 8 or 16) candidates per row and column split. */
#define WSAE_MATCH_COSINE 0
#define WSAE_MATCH_DOT 1
#define WSAE_MATCH_MAX_N 16
int64_t wsae_match_workspace_bytes(int32_t rows_a, int32_t rows_b, int32_t dim, int32_t top_n, int32_t precision);
int wsae_match_rows(const float* A, int32_t rows_a, int64_t lda, const float* B, int32_t rows_b, int64_t ldb,
                    int32_t dim, int32_t metric, int32_t precision, int32_t top_n, int32_t exclude_self,
                    float* out_val, int32_t* out_idx, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- co-activation statistics: co-firing counts and top partners -------------------------------
 * Over a stream of rows of two compact codes A [n_rows, k_a] and B [n_rows, k_b] (as wsae_encode_topk writes them; k_a
 * and k_b independent, each in 1..WSAE_COACT_MAX_K), count for every pair (feature i of A, feature j of B) the rows on
 * which both fire, then pick per feature of A the strongest partners under a normalised score.  Ctx-free; the caller's
 * stream, no allocation, no host synchronisation, no float atomics.  All state is integer: the results are identical
 * for any launch geometry, any order of the rows and any split of the rows over calls.
 * State (caller-owned, zero-initialised device memory): counts int32 [a_rows, ldc] (ldc >= hidden_b; columns from
 * hidden_b on are never touched), fire_a int32 [hidden_a], fire_b int32 [hidden_b] (nullable in the update),
 * total_rows int64 [1].
 * wsae_coact_update.  An entry is active iff v > 0 and 0 <= idx < hidden (masked BatchTopK entries carry v = 0; an
 * index outside the range is ignored).  A row with row_mask[r] == 0 contributes nothing (row_mask NULL: every row
 * does).  Per contributing row: total_rows += 1; fire_a[i] += 1 per active entry of A, whatever the window;
 * fire_b[j] += 1 per active entry of B; counts[i - a_lo][j] += 1 for every pair of an active entry of A with
 * a_lo <= i < a_lo + a_rows and an active entry of B (a repeated index counts once per occurrence).  vals_b / idx_b
 * may be the buffers of A: the table is then symmetric and its diagonal equals fire_a.  The window (a_lo, a_rows) lets
 * a large pair of dictionaries be processed in passes over row ranges of the table.  0 <= n_rows <= 2^31 - 1 per call;
 * keeping the cumulative total below 2^31 is the caller's job.
 * wsae_coact_top.  For every window row r (i = a_lo + r; c = counts[r][j], n = fire_a[i], m = fire_b[j],
 * N = *total_rows, read on the device) the top_n <= WSAE_MATCH_MAX_N best columns; the score matrix is never written.
 * Scores are fp64 from the integers with correctly rounded IEEE operations, rounded once to fp32:
 *   WSAE_COACT_COUNT    c
 *   WSAE_COACT_COND     c / n                      (0 if n == 0)
 *   WSAE_COACT_JACCARD  c / (n + m - c)            (denominator in int64; 0 if it is 0)
 *   WSAE_COACT_PHI      double(N c - n m) / (sqrt(double(n (N - n))) * sqrt(double(m (N - m))))
 *                                                  (products in int64; 0 if either product under a root is 0)
 * A column is a candidate iff j < hidden_b, c >= min_count (min_count >= 0) and, with exclude_self != 0, j != i.
 * Order: fp32 value descending, then index ascending (total, so independent of geometry).  With fewer than top_n
 * candidates the tail is val = -inf, idx = -1, cnt = 0.  out_cnt (nullable) receives c of each selected pair; fire_b
 * may be NULL for the COUNT and COND metrics.  Both workspace queries return 0 (neither call needs scratch; workspace
 * may be NULL) and -1 for invalid arguments. */
#define WSAE_COACT_COUNT 0
#define WSAE_COACT_COND 1
#define WSAE_COACT_JACCARD 2
#define WSAE_COACT_PHI 3
#define WSAE_COACT_MAX_K 128
int64_t wsae_coact_workspace_bytes(int64_t n_rows, int32_t k_a, int32_t hidden_a, int32_t k_b, int32_t hidden_b,
                                   int32_t a_lo, int32_t a_rows);
int wsae_coact_update(const float* vals_a, const int32_t* idx_a, int32_t k_a, int32_t hidden_a, const float* vals_b,
                      const int32_t* idx_b, int32_t k_b, int32_t hidden_b, int64_t n_rows, const uint8_t* row_mask,
                      int32_t a_lo, int32_t a_rows, int32_t* counts, int64_t ldc, int32_t* fire_a, int32_t* fire_b,
                      int64_t* total_rows, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_coact_top_workspace_bytes(int32_t a_lo, int32_t a_rows, int32_t hidden_b, int32_t top_n);
int wsae_coact_top(const int32_t* counts, int64_t ldc, int32_t a_lo, int32_t a_rows, int32_t hidden_b,
                   const int32_t* fire_a, const int32_t* fire_b, const int64_t* total_rows, int32_t metric,
                   int32_t min_count, int32_t exclude_self, int32_t top_n, float* out_val, int32_t* out_idx,
                   int32_t* out_cnt, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- group effect sizes: utterance pooling and bootstrap Cohen's d ------------------------------
 * Which features separate two groups of utterances, and how surely.  Ctx-free; the caller's stream, no allocation, no
 * host synchronisation, no float atomics; argument errors are found on the host before any HIP call.
 * wsae_pool_update.  Segment pooling of a compact code vals / idx [n_rows, k] (as wsae_encode_topk writes them,
 * 1 <= k <= WSAE_POOL_MAX_K).  seg int32 [n_rows] names the segment (utterance) of each row; a row with seg < 0 or
 * seg >= n_seg contributes nothing (padding frames).  The remaining values are expected to be non-decreasing within a
 * call (the frames of an utterance arrive together); where they are not, the result is the same and the call slower.
 * State (caller-owned, zero-initialised device memory): pooled_sum fp32 [n_seg, ld], pooled_cnt int32 [n_seg, ld]
 * (nullable), seg_rows int32 [n_seg]; ld >= f_cols, columns from f_cols on are never touched.  An entry is active iff
 * v > 0 and 0 <= idx < hidden (the rule of wsae_coact_update).  Per contributing row seg_rows[s] += 1; per active entry
 * with f_lo <= idx < f_lo + f_cols: pooled_sum[s][idx - f_lo] += v and pooled_cnt[s][idx - f_lo] += 1.
 * pooled_sum[s][f] is the fp32 sum in ascending row order (within a row: ascending entry position, which only matters
 * for an index repeated within a row), starting from the value already stored: a segment split over two calls, or any
 * launch geometry, gives the same bits, and sequential float32 adds reproduce them.  0 <= n_rows <= 2^31 - 1 per call.
 * Workspace: wsae_pool_workspace_bytes (8 n_seg bytes: the first and last row of each segment; -1 for invalid
 * arguments), contents arbitrary on entry.
 * wsae_group_effect.  Effect sizes of two groups of segments in fp64.  X fp32 [n_seg, ld] (the pooled_sum state, or any
 * dense per-utterance matrix), div int32 [n_seg] (nullable = 1): x_sf = double(X[s][f]) / div[s], a segment with
 * div[s] <= 0 is left out.  group int32 [n_seg]: 0 = group a, 1 = group b, anything else is ignored.  Per feature
 * f < f_cols, over the included members (n_a, n_b of them): the means, the unbiased variances by two passes,
 * s_p = sqrt(((n_a - 1) var_a + (n_b - 1) var_b) / (n_a + n_b - 2)), d = (mean_a - mean_b) / s_p (0 if s_p == 0),
 * g = d (1 - 3 / (4 (n_a + n_b) - 9)).  With n_a < 2 or n_b < 2 every fp64 output is NaN.
 * boot int16 [n_boot, n_seg] (nullable: n_boot = 0; else 2 <= n_boot <= WSAE_BOOT_MAX_R): resampling weights, negative
 * ones count as 0.  Per replicate and group: N = sum w, z = x - mean_g (the observed mean), S1 = sum w z,
 * S2 = sum w z^2, mean* = mean_g + S1 / N, var* = max(S2 - S1^2 / N, 0) / (N - 1), d* as above; a replicate with either
 * N < 2 is dropped.  Over the kept replicates (R' of them), sorted: ci_lo / ci_hi are the alpha / 2 and 1 - alpha / 2
 * quantiles by linear interpolation at position (R' - 1) q, se the sample standard deviation (n - 1, two passes).
 * Without boot ci_lo, ci_hi and se are NaN.  0 < alpha < 1.
 * Outputs: fp64 [f_cols] each mean_a, mean_b, d, g, ci_lo, ci_hi, se; record int32 [3] = n_a, n_b, kept replicates.
 * Every sum over segments runs in one fixed order per (replicate, feature): the result of a column depends on that
 * column, div, group and boot alone - not on the tile it sits in, its neighbours or ld - and two calls give the same
 * bits.  1 <= n_seg <= 2^20.  Workspace (16-byte aligned): wsae_group_effect_workspace_bytes - the segment selectors,
 * the replicate totals and the weights transposed to [segment][replicate]; -1 for invalid arguments. */
#define WSAE_POOL_MAX_K 128
#define WSAE_BOOT_MAX_R 2048
int64_t wsae_pool_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_seg, int32_t f_lo, int32_t f_cols);
int wsae_pool_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                     int32_t n_seg, int32_t f_lo, int32_t f_cols, float* pooled_sum, int32_t* pooled_cnt, int64_t ld,
                     int32_t* seg_rows, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_group_effect_workspace_bytes(int32_t n_seg, int32_t f_cols, int32_t n_boot);
int wsae_group_effect(const float* X, int64_t ld, const int32_t* div, const int32_t* group, int32_t n_seg, int32_t f_cols,
                      const int16_t* boot, int32_t n_boot, double alpha, double* mean_a, double* mean_b, double* d, double* g,
                      double* ci_lo, double* ci_hi, double* se, int32_t* record, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* ---- temporal run statistics: run lengths, gaps and event lists -----------------------------------
 * How long a feature stays on, how long it stays away and where in the utterance it fires, straight from a compact code
 * vals / idx [n_rows, k] (as wsae_encode_topk writes them, 1 <= k <= WSAE_RUNS_MAX_K) whose rows are in time order.
 * Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are found on
 * the host before any HIP call.  seg int32 [n_rows] names the segment (utterance) of each row; a row with seg < 0 or
 * seg >= n_seg is padding.  Feature f is active on row r iff some entry of the row has idx == f, v > 0 and
 * 0 <= f < hidden (the rule of wsae_coact_update); an index repeated within a row counts once, with the value of its
 * first active entry.  A run of f in segment s is a maximal set of rows a..b with consecutive row numbers, all of them
 * of segment s, on all of which f is active: a padding row or a row of another id ends a run, and so does the call
 * (segments are local to a call; pass whole utterances).  Its length is d = b - a + 1, its start a - (the first row of s
 * in the call), its total the fp32 sum of its values in ascending row order (sequential float32 adds reproduce it), its
 * peak their maximum.  Between two consecutive runs of f in the same segment lies a gap g = a_next - b_prev - 1 >= 1, a
 * difference of row numbers whatever lies between.  Both histograms have WSAE_RUNS_BINS bins: x <= 32 falls into bin
 * x - 1, a larger x into bin min(32 + floor(log2(x - 1)) - 5, 47), i.e. bin 32 + j holds (2^(5+j), 2^(6+j)].
 * State (caller-owned, zero-initialised device memory), per feature of the window f_lo <= f < f_lo + f_cols: frames
 * int32 (sum of d), runs int32, dur_max int32, dur_sq int64 (sum of d^2), dur_hist int32 [f_cols, 48], gap_hist int32
 * [f_cols, 48] (nullable); total_rows int64 [1] += the non-padding rows.  Every field is an integer sum or maximum
 * updated with integer atomics: the state does not depend on the launch geometry, on the order of the calls or on how
 * whole utterances are grouped into calls.
 * Events (ev_count nullable = none).  Every run with d >= ev_min_len (>= 1) takes a slot from the cursor ev_count int64
 * [1]; a slot below ev_cap receives ev_int [slot] = (feature, seg_base + s, start, d) and ev_flt [slot] = (total, peak)
 * (ev_int int32 [ev_cap, 4], ev_flt fp32 [ev_cap, 2]; with ev_cap == 0 both may be NULL and the call only counts).  The
 * cursor keeps counting past the capacity, so the caller sees how many records were dropped; the statistics do not
 * depend on the event arguments.  Records arrive in no particular order: sort by (feature, segment, start), which is
 * unique.  0 <= n_rows <= 2^31 - 1 per call.  Workspace: wsae_runs_workspace_bytes (8 n_seg bytes: the first and last
 * row of each segment; -1 for invalid arguments), contents arbitrary on entry. */
#define WSAE_RUNS_MAX_K 128
#define WSAE_RUNS_BINS 48
int64_t wsae_runs_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_seg, int32_t f_lo, int32_t f_cols);
int wsae_runs_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                     int32_t n_seg, int32_t seg_base, int32_t f_lo, int32_t f_cols, int32_t* frames, int32_t* runs,
                     int32_t* dur_max, int64_t* dur_sq, int32_t* dur_hist, int32_t* gap_hist, int64_t* total_rows,
                     int32_t* ev_int, float* ev_flt, int64_t ev_cap, int32_t ev_min_len, int64_t* ev_count, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- feature-triggered averages of a per-frame signal ---------------------------------------------
 * What is in the input when a feature fires: the average of a dense per-frame signal (log-mel frames, another layer's
 * residual, a one-hot alignment) around the rows on which a feature is active, straight from a compact code vals / idx
 * [n_rows, k] (as wsae_encode_topk writes them, 1 <= k <= WSAE_STA_MAX_K) whose rows are in time order.  Ctx-free; the
 * caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are found on the host
 * before any HIP call.  seg int32 [n_rows] (nullable = one segment) names the segment (utterance) of each row; a row
 * with seg < 0 is padding.  y [n_rows, ldy] of y_dtype WSAE_DT_F32 or WSAE_DT_BF16 is the signal: `channels` columns
 * (1 <= channels <= WSAE_STA_MAX_CH, ldy >= channels), columns from `channels` on are never read.  Lags
 * -1024 <= lag_lo <= lag_hi <= 1024, L = lag_hi - lag_lo + 1 <= WSAE_STA_MAX_LAGS; 0 need not be among them.
 * Triggers.  Feature f is active on row r iff the row is not padding and some entry has idx == f, v > 0 and
 * 0 <= f < hidden (the rule of wsae_runs_update); an index repeated within a row counts once, with the value of its
 * first active entry.  WSAE_STA_TRIGGER_ALL: every active (row, feature) is a trigger.  WSAE_STA_TRIGGER_ONSET: only
 * where r == 0, or seg[r - 1] != seg[r], or f is not active on row r - 1.  The weight w of a trigger is v
 * (WSAE_STA_WEIGHT_VALUE) or 1 (WSAE_STA_WEIGHT_ONE).
 * Terms.  Trigger (r, f) has a term at lag l iff 0 <= r + l < n_rows and seg[r + l] == seg[r]: lags never cross an
 * utterance, the signal of a padding row is never read, and a call sees whole utterances.
 * State (caller-owned, zero-initialised device memory), per feature of the window f_lo <= f < f_lo + f_cols: acc fp64
 * [f_cols, L, channels], wsum fp64 [f_cols, L], cnt int64 [f_cols, L].  Every term adds double(w) * double(y[r + l][c])
 * (exact in fp64) to acc[f][l][c], double(w) to wsum[f][l] and 1 to cnt[f][l].  Each cell of acc and wsum is ONE chain
 * of fp64 additions in ascending trigger row, starting from the stored value: a sequential fp64 loop reproduces the
 * bits, and they do not depend on the launch geometry, on the tile or window a feature sits in, on ldy, or on how whole
 * utterances are grouped into calls as long as they arrive in the same order.  0 <= n_rows <= 2^31 - 1 per call.
 * Workspace (8-byte aligned): wsae_sta_workspace_bytes - the per-feature trigger lists (8 n_rows k bytes), the
 * [chunks, f_cols] count table and three vectors of f_cols; -1 for invalid arguments; contents arbitrary on entry. */
#define WSAE_STA_TRIGGER_ALL 0
#define WSAE_STA_TRIGGER_ONSET 1
#define WSAE_STA_WEIGHT_VALUE 0
#define WSAE_STA_WEIGHT_ONE 1
#define WSAE_STA_MAX_K 128
#define WSAE_STA_MAX_LAGS 64
#define WSAE_STA_MAX_CH 4096
int64_t wsae_sta_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols);
int wsae_sta_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                    const void* y, int32_t y_dtype, int32_t channels, int64_t ldy, int32_t lag_lo, int32_t lag_hi,
                    int32_t f_lo, int32_t f_cols, int32_t trigger, int32_t weight, double* acc, double* wsum, int64_t* cnt,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- activation profiles: value histograms and stratified samples ----------------------------------
 * What the distribution of a feature's activations looks like, and examples drawn uniformly from every band of it,
 * straight from a compact code vals / idx [n_rows, k] (as wsae_encode_topk writes them, 1 <= k <= WSAE_PROFILE_MAX_K).
 * Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are found on
 * the host before any HIP call.  seg int32 [n_rows] (nullable = no padding): a row with seg < 0 is padding.  Feature f is
 * active on a row iff the row is not padding and some entry has idx == f, v > 0 and 0 <= f < hidden (the rule of
 * wsae_runs_update); an index repeated within a row counts once, with the value of its first active entry.  NaN is never
 * active, +inf is.  The window is f_lo <= f < f_lo + f_cols; 0 <= n_rows <= 2^31 - 1 per call.
 *
 * wsae_profile_update.  With b the int32 bit pattern of an active value v, its bin is clamp((b >> 20) - 920, 0, 191):
 * WSAE_PROFILE_BINS = 192 bins, eight per octave over [2^-12, 2^12); bin 8 e + s holds
 * [2^(e-12) (1 + s/8), 2^(e-12) (1 + (s+1)/8)), bin 0 also everything below 2^-12 (denormals included) and bin 191
 * everything from 4096 on.  State (caller-owned device memory, zero-initialised except min_bits), per feature of the
 * window: fires int32 (the rows on which it was active), hist int32 [f_cols, 192], max_bits int32 (the maximum of b;
 * positive floats order as their bits), min_bits int32 (the minimum; initialise to 0x7f800000), over int32 (values
 * >= 4096), sum_q int64 (the sum of rint(min(v, 4096) 2^20): the product is exact in fp32, the conversion rounds to
 * nearest even; a term is at most 2^32, so 2^31 - 1 rows cannot overflow it); total_rows int64 [1] += the non-padding
 * rows.  Every field is an integer sum, minimum or maximum: the state does not depend on the launch geometry, on the
 * order of the calls or on the batching, and two states merge by add / min / max.  Workspace:
 * wsae_profile_workspace_bytes, 0 for valid arguments in this form (NULL is accepted then) and -1 for invalid ones.
 *
 * wsae_sample_update.  Row r of the call has the ordinal ord_base + r (0 <= ord_base, ord_base + n_rows <= 2^31; padding
 * rows take their ordinal too).  edges fp32 [f_cols, n_strata - 1], ascending per feature of the window (1 <= n_strata <=
 * WSAE_SAMPLE_MAX_STRATA; NULL allowed when n_strata == 1): the stratum of an active (row, f, v) is the number of f's
 * edges that are <= v.  Its priority, in uint32 arithmetic with o the ordinal:
 *     x = o * 0x9E3779B1 ^ f * 0x85EBCA77 ^ seed;  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;
 *     x ^= x >> 16
 * (f is the feature's index in [0, hidden), not its column in the window) and its key is (uint64) x << 32 | o, unique
 * within a feature.  State per list (feature of the window, stratum): keys uint64 [f_cols, n_strata, keep] ascending,
 * an unused slot = 2^64 - 1 (the caller initialises them so; no key reaches it); svals fp32 [f_cols, n_strata, keep],
 * the values beside the keys, 0 in an unused slot; seen int32 [f_cols, n_strata] += every active entry of the stratum,
 * sampled or not (1 <= keep <= WSAE_SAMPLE_MAX_KEEP).  After any sequence of calls a list holds the `keep` smallest keys
 * ever offered to it: a uniform sample without replacement of the stratum that does not depend on call order, batching
 * or launch geometry, and two states over disjoint ordinals merge exactly (union, keep the smallest).  At most
 * 2^31 - 1 entries (n_rows k) per call and fewer than 2^31 - 1 lists (f_cols n_strata).  Workspace (8-byte aligned): wsae_sample_workspace_bytes - three int32 vectors
 * over the lists and 12 bytes per entry; -1 for invalid arguments; contents arbitrary on entry. */
#define WSAE_PROFILE_MAX_K 128
#define WSAE_PROFILE_BINS 192
#define WSAE_SAMPLE_MAX_STRATA 16
#define WSAE_SAMPLE_MAX_KEEP 64
int64_t wsae_profile_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols);
int wsae_profile_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                        int32_t f_lo, int32_t f_cols, int32_t* fires, int32_t* hist, int32_t* max_bits, int32_t* min_bits,
                        int32_t* over, int64_t* sum_q, int64_t* total_rows, void* workspace, int64_t workspace_bytes,
                        void* stream);
int64_t wsae_sample_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols, int32_t n_strata,
                                    int32_t keep);
int wsae_sample_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                       int64_t ord_base, int32_t f_lo, int32_t f_cols, const float* edges, int32_t n_strata, int32_t keep,
                       uint32_t seed, uint64_t* keys, float* svals, int32_t* seen, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---- label association: feature-by-class counts with lags -------------------------------------------
 * Which feature detects which class of a per-frame label, at which activation threshold and how many frames early or
 * late: integer counts per (feature, lag, class, value stratum) straight from a compact code vals / idx [n_rows, k]
 * (1 <= k <= WSAE_LABEL_MAX_K) and labels int32 [n_rows], in one pass.  Ctx-free; the caller's stream, no allocation, no
 * host synchronisation, no float atomics; argument errors are found on the host before any HIP call.
 *
 * Activity (the rule of wsae_profile_update): feature f is active on row r iff the row is not padding and some entry has
 * idx == f, v > 0 and 0 <= f < hidden; an index repeated within a row counts once, with the value of its first active
 * entry.  NaN is never active, +inf is.  seg int32 [n_rows] (nullable = one segment, no padding): a row with seg < 0 is
 * padding.  Stratum (the rule of wsae_sample_update): edges fp32 [f_cols, n_strata - 1], ascending per feature of the
 * window (1 <= n_strata <= WSAE_LABEL_MAX_STRATA; NULL allowed when n_strata == 1); the stratum of an active (r, f, v) is
 * the number of f's edges that are <= v; a NaN edge is never <= v.
 *
 * Pairs.  The lags are lag_lo .. lag_hi with -1024 <= lag_lo <= lag_hi <= 1024 and L = lag_hi - lag_lo + 1 <=
 * WSAE_LABEL_MAX_LAGS; lag 0 need not be among them.  (r, l) is a pair iff row r is not padding, 0 <= r + l < n_rows,
 * seg[r + l] == seg[r] and 0 <= labels[r + l] < n_classes (1 <= n_classes <= WSAE_LABEL_MAX_CLASSES); its class is
 * c = labels[r + l].  A label outside [0, n_classes) - -1 for "unlabelled" - drops the pair and nothing else.  Lags never
 * cross an utterance: a call sees whole utterances.
 *
 * State (caller-owned device memory, zero-initialised): pair_rows int64 [L, n_classes] += 1 per pair, whatever the
 * features do; cnt int32 [f_cols, L, n_classes, n_strata] += 1 per pair and per feature of the window
 * (f_lo <= f < f_lo + f_cols) active on row r, at [f - f_lo][l - lag_lo][c][stratum]; offsets are computed in 64 bits.
 * Every field is an integer sum: the state does not depend on the launch geometry, on the order of the calls or on the
 * grouping of whole utterances into calls, and two states add.  0 <= n_rows <= 2^31 - 1 per call; n_rows == 0 returns
 * WSAE_OK and touches nothing.  Workspace: wsae_label_workspace_bytes, 0 for valid arguments in this form (NULL is
 * accepted then) and -1 for invalid ones; contents arbitrary on entry. */
#define WSAE_LABEL_MAX_K 128
#define WSAE_LABEL_MAX_CLASSES 1024
#define WSAE_LABEL_MAX_LAGS 16
#define WSAE_LABEL_MAX_STRATA 16
int64_t wsae_label_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols,
                                   int32_t n_classes, int32_t lag_lo, int32_t lag_hi, int32_t n_strata);
int wsae_label_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                      const int32_t* labels, int64_t n_rows, int32_t n_classes, int32_t lag_lo, int32_t lag_hi,
                      int32_t f_lo, int32_t f_cols, const float* edges, int32_t n_strata, int32_t* cnt, int64_t* pair_rows,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- sparse linear probes: softmax regression on the compact code -----------------------------------
 * How well does a SET of features predict a per-frame label?  The two sparse products of one iteration of a softmax
 * regression over a compact code vals / idx [n_rows, k] (1 <= k <= WSAE_PROBE_MAX_K); the dense [n_rows, hidden] code
 * never exists.  Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics; argument
 * errors are found on the host before any HIP call; n_rows == 0 returns WSAE_OK and touches nothing; every
 * *_workspace_bytes returns -1 for invalid arguments; workspace contents are arbitrary on entry.
 *
 * Activity is the rule of wsae_profile_update (above): seg[r] >= 0 (NULL: one segment, no padding), some entry with
 * idx == f, v > 0 and 0 <= f < hidden; a repeated index counts once, with the value of its first active entry; NaN is
 * never active.  Columns: col_of int32 [hidden] maps a feature to its probe column in [0, n_cols), -1 = not in the probe;
 * NULL = the identity, and then n_cols == hidden.  A value outside [-1, n_cols) and two features on one column are the
 * caller's errors and are not detected.
 *
 * wsae_probe_plan transposes the code: one entry per active (row, feature) with a column, grouped by column and in
 * ascending row within a column (a stable counting sort).  col_ptr int64 [n_cols + 1], t_row int32 [cap], t_val fp32
 * [cap], nnz int64 [1].  col_ptr and nnz always describe ALL entries; slots from cap on are not written, so a caller who
 * finds nnz > cap grows the buffers and calls again.  The result depends on the code, seg and col_of only.
 *
 * wsae_probe_forward.  The label of row r is labels[r + lag] (-1024 <= lag <= 1024); it is valid iff r is not padding,
 * 0 <= r + lag < n_rows, seg[r + lag] == seg[r] and the label lies in [0, n_classes).  Otherwise the row is dropped: its
 * err row is exact zeros, its row_loss 0, it counts nowhere.  On a used row with label y
 *   logit[c] = bias[c] + sum_j v_j W[col_j][c]   over the row's first-active entries with a column, in ascending entry
 *              position; every step is an fp32 multiply and then an fp32 add (NOT fused), W fp32 [n_cols, ldw];
 *   m = max logit, e_c = expf(logit[c] - m), s = sum e_c, loss = w_y ((logf(s) + m) - logit[y]),
 *   err[c] = w_y (e_c / s - [c == y]),   w = class_weight fp32 [n_classes] (NULL: 1).
 * The maximum and the sum over classes are taken as 64 partials (partial l over the classes l, l + 64, ... ascending,
 * from -inf / 0) combined by a butterfly at distances 32, 16, 8, 4, 2, 1; what is written for a row depends on that row
 * alone.  Outputs, each nullable one skipped when NULL: err fp32 [n_rows, lde] (nullable; lde >= n_classes, columns from
 * n_classes on are never written); row_loss fp32 [n_rows] (nullable); n_used, n_correct (argmax == y, ties to the lowest
 * class), loss_q int64 [1] += llrint(min(loss, 1024) 2^20); confusion int64 [n_classes, n_classes] (nullable) += 1 at
 * [y][argmax].  The four are integer sums on caller-owned state: identical for any batching of whole utterances and any
 * call order, and two shards add.
 *
 * wsae_probe_backward: gW fp64 [n_cols, n_classes] and gb fp64 [n_classes] accumulate from the stored value.  With the
 * entries i = 0 .. n_p - 1 of column p (clipped to cap), partial_q[c] is ONE chain of fp64 additions, started at 0, of
 * double(t_val[i]) double(err[t_row[i]][c]) over i = q CHUNK .. min((q + 1) CHUNK, n_p) - 1 in order (CHUNK =
 * WSAE_PROBE_CHUNK; the product is exact), and gW[p][c] = ((stored + partial_0) + partial_1) + ...; a column without
 * entries is not touched.  gb[c] the same over chunks of CHUNK consecutive rows of the call with terms double(err[r][c]).
 * A sequential loop reproduces every bit; the result depends neither on the launch geometry nor on lde. */
#define WSAE_PROBE_MAX_K 128
#define WSAE_PROBE_MAX_CLASSES 1024
#define WSAE_PROBE_CHUNK 2048
int64_t wsae_probe_plan_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols);
int wsae_probe_plan(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                    const int32_t* col_of, int32_t n_cols, int64_t* col_ptr, int32_t* t_row, float* t_val, int64_t cap,
                    int64_t* nnz, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_probe_forward_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols, int32_t n_classes,
                                           int32_t lag);
int wsae_probe_forward(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                       const int32_t* labels, int64_t n_rows, int32_t lag, int32_t n_classes, const int32_t* col_of,
                       int32_t n_cols, const float* W, int64_t ldw, const float* bias, const float* class_weight, float* err,
                       int64_t lde, float* row_loss, int64_t* n_used, int64_t* n_correct, int64_t* loss_q, int64_t* confusion,
                       void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_probe_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_classes, int64_t cap);
int wsae_probe_backward(const int64_t* col_ptr, const int32_t* t_row, const float* t_val, int64_t cap, int32_t n_cols,
                        const float* err, int64_t lde, int32_t n_classes, int64_t n_rows, double* gW, double* gb,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- sparse ridge regression: the code's Gram matrix and the linear forward --------------------------
 * How well does a feature, or a set of features, track a CONTINUOUS per-frame quantity?  The sufficient statistics of a
 * linear regression on a compact code vals / idx [n_rows, k] (1 <= k <= WSAE_PROBE_MAX_K) are its Gram matrix G = X^T X and
 * the cross moment M = X^T Y; the dense [n_rows, hidden] code X never exists.  M is wsae_probe_backward with the target
 * rows in the place of err.  Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics;
 * argument errors are found on the host before any HIP call; n_rows == 0 returns WSAE_OK and touches nothing; every
 * *_workspace_bytes returns -1 for invalid arguments; workspace contents are arbitrary on entry.  Activity, padding
 * (seg[r] < 0; NULL: none) and col_of / n_cols are those of wsae_probe_plan (above).
 *
 * wsae_gram_update.  col_ptr / t_row / t_val / cap: the plan wsae_probe_plan made of this very code, seg and col_of.  With
 * u_c(r) the value with which column c is active on row r, and the entries i = 0 .. n_p - 1 of column p (clipped to cap),
 * partial_q[c] is ONE chain of fp64 additions, started at 0, of double(t_val[i]) double(u_c(t_row[i])) over
 * i = q CHUNK .. min((q + 1) CHUNK, n_p) - 1 in order (CHUNK = WSAE_PROBE_CHUNK), over those i only on whose row c is
 * active; the product of two fp32 values is exact in fp64.  For the rows p of the window p_lo <= p < p_lo + p_rows
 * (inside [0, n_cols)) and c >= p:  G[p - p_lo][c] = ((stored + partial_0) + partial_1) + ...;  G fp64 [p_rows, ldg],
 * ldg >= n_cols <= WSAE_GRAM_MAX_COLS.  Only the upper triangle is produced: cells with c < p and columns from n_cols on
 * are never written, and a column p without entries touches nothing.  On the diagonal u_p(r) is the very t_val[i].  An
 * entry whose t_row lies outside [0, n_rows) or on a padding row adds nothing.  A sequential loop reproduces every bit;
 * the result depends on the code, seg, col_of, the stored G and the sequence of calls - not on the launch geometry, ldg,
 * the split into row windows or the workspace.  Workspace (8-byte aligned): wsae_gram_workspace_bytes - 8 bytes per entry
 * of the code (n_rows k): every call first writes the column and the value of every entry there, once per row.
 *
 * wsae_regress_forward.  Y fp32 [n_rows, ldy] (nullable), 1 <= n_targets <= WSAE_PROBE_MAX_CLASSES; the target of row r is
 * Y[r + lag] (-1024 <= lag <= 1024).  Row r is USED iff it is not padding, 0 <= r + lag < n_rows, seg[r + lag] == seg[r]
 * and all n_targets values of Y[r + lag] are finite.  W fp64 [n_cols, ldw], bias fp64 [n_targets]:
 *   yhat[c] = bias[c], then + double(v_j) W[col_j][c] over the row's first-active entries with a column, in ascending
 *             entry position; every step is an fp64 multiply and then an fp64 add (NOT fused).
 * pred fp32 [n_rows, ldp] (nullable; columns from n_targets on are never written) = float(yhat) on every non-padding row,
 * used or not, and exact zeros on a padding row.  With Y: n_used int64 [1] += the used rows (an integer sum); stats fp64
 * [5, n_targets] accumulates sum y, sum y^2, sum yhat, sum yhat^2, sum (y - yhat)^2 over the used rows, yhat in fp64 and
 * every square an fp64 multiply: per cell and chunk of CHUNK consecutive rows of the call ONE chain of fp64 additions
 * from 0 in row order (unused rows add nothing), and stats = ((stored + partial_0) + partial_1) + ...  With Y == NULL only
 * pred is written (and is required).  Workspace (8-byte aligned): wsae_regress_forward_workspace_bytes - 40 bytes per
 * chunk and target; not needed when Y == NULL. */
#define WSAE_GRAM_MAX_COLS 8192
int64_t wsae_gram_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols, int32_t p_rows, int64_t cap);
int wsae_gram_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                     const int32_t* col_of, int32_t n_cols, const int64_t* col_ptr, const int32_t* t_row, const float* t_val,
                     int64_t cap, int32_t p_lo, int32_t p_rows, double* G, int64_t ldg, void* workspace,
                     int64_t workspace_bytes, void* stream);
int64_t wsae_regress_forward_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols, int32_t n_targets,
                                             int32_t lag);
int wsae_regress_forward(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, const float* Y,
                         int64_t ldy, int64_t n_rows, int32_t lag, int32_t n_targets, const int32_t* col_of, int32_t n_cols,
                         const double* W, int64_t ldw, const double* bias, float* pred, int64_t ldp, int64_t* n_used,
                         double* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- code dynamics: frame similarity and boundary scoring --------------------------------------------
 * How the code of a frame as a whole moves through time: the similarity of the codes of frames r and r + l straight from
 * a compact code vals / idx [n_rows, k] (1 <= k <= WSAE_DYN_MAX_K) whose rows are in time order, and the score of a
 * per-frame boundary curve against reference boundaries at every threshold.  Ctx-free; the caller's stream, no
 * allocation, no host synchronisation, no float atomics; argument errors are found on the host before any HIP call;
 * n_rows == 0 returns WSAE_OK and touches nothing; every *_workspace_bytes returns -1 for invalid arguments; workspace
 * contents are arbitrary on entry.
 *
 * Active entries (the rule of wsae_runs_update).  seg int32 [n_rows] (nullable = one segment, no padding): a row with
 * seg < 0 is padding.  Feature f is active on row r iff the row is not padding and some entry has idx == f, v > 0 (NaN is
 * not, +inf is) and 0 <= f < hidden; an index repeated within a row counts once, with the value of its first active
 * entry.  weight fp32 [hidden] (nullable = all 1): the feature's value on the row is u = v weight[f], one fp32 product,
 * and a feature with weight[f] <= 0 or NaN is active on no row.  Without weight u = v.
 *
 * wsae_dyn_update.  lags int32 [n_lags] in HOST memory: ascending, distinct, 1 <= lag <= WSAE_DYN_MAX_LAG,
 * 1 <= n_lags <= WSAE_DYN_MAX_LAGS.  The pair of (r, lag l) is (r, q = r + l); it is valid iff row r is not padding,
 * q < n_rows and seg[q] == seg[r] (without seg: iff q < n_rows).  The rows in between are not examined.  With p the
 * entry positions 0 .. k - 1 of row r in ascending order, restricted to the positions that hold an active feature of r:
 *   s   = ONE chain of fp64 additions from 0 of double(u_r(f_p)) double(u_q(f_p)) over those p whose feature is active on
 *         row q as well (the product of two fp32 values is exact in fp64);
 *   n_r = ONE chain of fp64 additions from 0 of double(u_r(f_p))^2 over all those p (n_q likewise over the positions of q);
 *   a_r = the number of active features of row r, i = the number of those p that matched.
 * WSAE_DYN_DOT: s.  WSAE_DYN_COSINE: 0 where n_r == 0 or n_q == 0, else c = s / sqrt(n_r n_q) in fp64 (one product, one
 * square root, one quotient) and 1 unless c <= 1.  WSAE_DYN_JACCARD: 0 where a_r + a_q - i == 0, else the fp64 quotient
 * i / (a_r + a_q - i).  The result is rounded once to fp32.  A sequential loop reproduces every bit; the value does not
 * depend on the launch geometry, on the other lags of the call or on how whole utterances are grouped into calls.
 *   sim fp32 [n_rows, n_lags] (nullable): the similarity of a valid pair, NaN for an invalid one.
 *   State (nullable as a whole: pairs, sim_q, sq_q, hist and total_rows all or none; caller-owned, zero-initialised
 *   device memory; WSAE_DYN_COSINE and WSAE_DYN_JACCARD only - with WSAE_DYN_DOT it is WSAE_ERR_INVALID).  label int32
 *   [n_rows] (nullable = no frame is labelled; a label < 0 is "unlabelled").  The class of a valid pair: 0 = both frames
 *   labelled and equal, 1 = both labelled and different, 2 = otherwise.  With x = llrint(double(sim) 2^30) (exact; 0 <= x
 *   <= 2^30), cell [l][class] of pairs int64 [n_lags, 3] += 1, of sim_q int64 [n_lags, 3] += x, of sq_q int64 [n_lags, 3]
 *   += (x >> 15)^2, and hist int64 [n_lags, 3, WSAE_DYN_BINS] += 1 at bin min(x >> 24, 63); total_rows int64 [1] += the
 *   non-padding rows.  Every field is an integer sum: two states add, whatever the order of the calls.
 * Workspace (8-byte aligned): wsae_dyn_workspace_bytes - the canonical code (8 bytes per entry: u, and f or -1) and 12
 * bytes per row (n_r, a_r), in sections of 256-byte multiples.
 *
 * wsae_boundary_score.  nov fp32 [n_rows]: nov[r] describes the boundary between rows r and r + 1, NaN = undefined.  ref
 * uint8 [n_rows] (nullable = no references): nonzero = a reference boundary at r.  thr fp32 [n_thr] in DEVICE memory,
 * 1 <= n_thr <= WSAE_BOUNDARY_MAX_THR, in any order, equal values, infinities and NaN (which predicts nothing) allowed;
 * 0 <= tol <= WSAE_BOUNDARY_MAX_TOL rows.  A stretch is a maximal run of consecutive rows with equal seg >= 0 (without
 * seg: the whole call).  Row r of a stretch is a peak iff nov[r] > left and nov[r] >= right, where a neighbour that lies
 * in another stretch, outside the call or is NaN counts as -inf (so a NaN or -inf row is no peak, and a plateau peaks at
 * its first row).  At threshold t the predictions of a stretch are its peaks with nov >= t, the references its rows
 * with ref != 0, and the hits the greedy one-to-one match of the two lists in time order: with p and q the earliest
 * prediction and reference not yet consumed, |p - q| <= tol is a hit that consumes both, otherwise the earlier of the two
 * is consumed.  n_pred int64 [n_thr] += the predictions, n_hit int64 [n_thr] += the hits, n_ref int64 [1] += the
 * references, n_peaks int64 [1] += the peaks (all stretches of the call; integer sums, so calls add); peaks uint8
 * [n_rows] (nullable) = 1 on a peak and 0 elsewhere, written on every row.  Workspace (8-byte aligned):
 * wsae_boundary_workspace_bytes - one flag byte and one stretch-list slot of 4 bytes per row, and a counter. */
#define WSAE_DYN_COSINE 0
#define WSAE_DYN_DOT 1
#define WSAE_DYN_JACCARD 2
#define WSAE_DYN_MAX_K 128
#define WSAE_DYN_MAX_LAGS 16
#define WSAE_DYN_MAX_LAG 1024
#define WSAE_DYN_BINS 64
#define WSAE_BOUNDARY_MAX_THR 256
#define WSAE_BOUNDARY_MAX_TOL 64
int64_t wsae_dyn_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_lags);
int wsae_dyn_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, const float* weight,
                    const int32_t* label, int64_t n_rows, const int32_t* lags, int32_t n_lags, int32_t metric, float* sim,
                    int64_t* pairs, int64_t* sim_q, int64_t* sq_q, int64_t* hist, int64_t* total_rows, void* workspace,
                    int64_t workspace_bytes, void* stream);
int64_t wsae_boundary_workspace_bytes(int64_t n_rows, int32_t n_thr, int32_t tol);
int wsae_boundary_score(const float* nov, const int32_t* seg, const uint8_t* ref, int64_t n_rows, const float* thr,
                        int32_t n_thr, int32_t tol, int64_t* n_pred, int64_t* n_hit, int64_t* n_ref, int64_t* n_peaks,
                        uint8_t* peaks, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- code clustering: k-means on the compact code -----------------------------------------------------
 * Do the frames fall into a few hundred discrete units?  The two halves of a Lloyd iteration over a compact code vals /
 * idx [n_rows, k] (1 <= k <= WSAE_CLUSTER_MAX_K) and 1 <= n_clusters <= WSAE_CLUSTER_MAX centroids; neither the dense
 * [n_rows, hidden] code nor a [n_rows, n_clusters] product exists.  Ctx-free; the caller's stream, no allocation, no host
 * synchronisation, no float atomics; argument errors are found on the host before any HIP call; n_rows == 0 returns
 * WSAE_OK and touches nothing; every *_workspace_bytes returns -1 for invalid arguments (and 0 otherwise: neither call
 * keeps anything); workspace contents are arbitrary on entry.  Activity, padding (seg[r] < 0; NULL: none) and col_of /
 * n_cols are those of wsae_probe_plan (above).
 *
 * wsae_cluster_assign.  Ct fp32 [n_cols, ldc] (ldc >= n_clusters): the centroids TRANSPOSED - the row of a column holds
 * its weight in every cluster, the layout of the probe's W.  bias fp32 [n_clusters] (nullable = 0).  On a row that is not
 * padding and has at least one first-active entry with a column
 *   score[c] = bias[c], then + v_j Ct[col_j][c] over those entries in ascending entry position; every step is an fp32
 *              multiply and then an fp32 add (NOT fused);
 *   a        = the lowest c at the maximum score, best = score[a];
 *   second   = score[a2], a2 the lowest c != a at the maximum over c != a; -inf when n_clusters == 1;
 *   n        = ONE chain of fp64 additions from 0 of double(v_j)^2 over the same entries in the same order;
 *   inv_norm = float(1.0 / sqrt(n)): one fp64 root, one fp64 quotient, one rounding;
 *   b        = best inv_norm (one fp32 product) with normalize != 0, which needs bias == NULL (WSAE_ERR_INVALID
 *              otherwise); b = best without.
 * Finite Ct and bias are the caller's duty.  Outputs, each nullable and skipped when NULL: assign int32 [n_rows] = a, and
 * -1 on a padding row and on a row without such an entry (an EMPTY row); best, second, inv_norm fp32 [n_rows], exact
 * zeros where assign is -1.  State, each nullable and skipped when NULL, integer sums on caller-owned device memory:
 * count int64 [n_clusters] += 1 at a; best_q int64 [n_clusters] += llrintf(fminf(fmaxf(b, -4096), 4096) 2^20) at a;
 * contingency int64 [n_clusters, n_classes] += 1 at [a][labels[r]] where the label lies in [0, n_classes) (labels int32
 * [n_rows], nullable; with labels 1 <= n_classes <= WSAE_CLUSTER_MAX, and a contingency table needs labels); totals int64
 * [3] += the assigned rows, the empty rows, the assigned rows with a label in range.  What is written for a row depends
 * on that row alone; the sums are identical for any batching and any call order, and two shards add.  Cosine (spherical)
 * k-means: unit centroids, normalize = 1, no bias.  Euclidean k-means: bias[c] = -|c|^2 / 2, since argmin |x - c|^2 is the
 * argmax of this score.
 *
 * wsae_cluster_accumulate.  col_ptr / t_row / t_val / cap / n_cols: the plan wsae_probe_plan made of this very code, seg
 * and col_of.  assign int32 [n_rows]; row_weight fp32 [n_rows] (nullable; for cosine the inv_norm of the assign call);
 * S_q int64 [n_cols, lds] (lds >= n_clusters), the orientation of Ct.  Entry i of column p (the lists clipped to cap),
 * with r = t_row[i] and x = t_val[i], or the one fp32 product t_val[i] row_weight[r], adds
 * llrintf(fminf(x, 4096) 2^20) to S_q[p][assign[r]]; nothing where r is outside [0, n_rows), assign[r] is outside
 * [0, n_clusters) or x is not > 0 (NaN is not).  Integer sums: bit-identical for any launch geometry, any batching and
 * any call order; the states of two shards add.  The centroid of cluster c is S_q[.][c] / (count[c] 2^20). */
#define WSAE_CLUSTER_MAX_K 128
#define WSAE_CLUSTER_MAX 1024
int64_t wsae_cluster_assign_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols, int32_t n_clusters);
int wsae_cluster_assign(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, int64_t n_rows,
                        const int32_t* col_of, int32_t n_cols, const float* Ct, int64_t ldc, const float* bias,
                        int32_t n_clusters, int32_t normalize, const int32_t* labels, int32_t n_classes, int32_t* assign,
                        float* best, float* second, float* inv_norm, int64_t* count, int64_t* best_q, int64_t* contingency,
                        int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_cluster_accumulate_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_clusters, int64_t cap);
int wsae_cluster_accumulate(const int64_t* col_ptr, const int32_t* t_row, const float* t_val, int64_t cap, int32_t n_cols,
                            const int32_t* assign, const float* row_weight, int64_t n_rows, int32_t n_clusters, int64_t* S_q,
                            int64_t lds, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- ABX phone discrimination: DTW distances between segments and the triple count --------------------
 * Is a token X of a phone closer to another token A of the same phone than to a token B of another one?  "Closer" is the
 * DTW-aligned frame distance between two row ranges of a compact code vals / idx [n_rows, k] (1 <= k <= WSAE_DTW_MAX_K).
 * Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are found on
 * the host before any HIP call; every *_workspace_bytes returns -1 for invalid arguments; workspace contents are
 * arbitrary on entry.
 *
 * wsae_dtw_matrix.  Activity, padding (seg[r] < 0; seg nullable), weight, u = v weight[f] and the per-row quantities n_r
 * and a_r are exactly those of wsae_dyn_update (above): an index repeated within a row counts once, with the value of its
 * first active entry.  Items are row ranges [start, start + len) of this one code; a_start / a_len int32 [n_a] and
 * b_start / b_len int32 [n_b] in DEVICE memory.  An item is valid iff 1 <= len <= WSAE_DTW_MAX_LEN, start >= 0 and
 * start + len <= n_rows; items may overlap and repeat.  For frame r of an a-item and frame q of a b-item - any two rows,
 * there is no same-segment condition - with p the entry positions 0 .. k - 1 of row q (the B frame) in ascending order,
 * restricted to the positions that hold an active feature of q which is active on r as well:
 *   s = ONE chain of fp64 additions from 0 of double(u_q(f_p)) double(u_r(f_p)) over those p; i = their number.
 * WSAE_DTW_COSINE: c = 0 where n_r == 0 or n_q == 0, else c = s / sqrt(n_r n_q) in fp64 (one product, one square root, one
 * quotient) and 1 unless c <= 1.  WSAE_DTW_JACCARD: c = 0 where a_r + a_q - i == 0, else the fp64 quotient
 * i / (a_r + a_q - i); it needs presence, not values (a u that underflowed to 0 counts).  The frame cost is
 * e = float(1.0 - c): one fp64 subtraction, one rounding.
 * The dynamic program of an a-item of n frames and a b-item of m frames: D[0][0] = double(e[0][0]), L[0][0] = 1; every
 * other cell takes the predecessor with the smallest D among those that exist, (i-1, j-1), (i-1, j), (i, j-1), ties to
 * the earlier one in that order; D[i][j] = double(e[i][j]) + D[pred] (one fp64 addition), L[i][j] = L[pred] + 1.
 *   dist fp32 [n_a, ldd] (ldd >= n_b): float(D[n-1][m-1] / double(L[n-1][m-1])) with normalize != 0 (the path-length
 *   normalisation of the ABX literature), float(D[n-1][m-1]) without; steps int32 [n_a, ldd] (nullable): L[n-1][m-1].
 *   A pair with an invalid item gets NaN and 0.  Every cell [a][b < n_b] is written and nothing beyond column n_b of a row.
 * A sequential loop reproduces every bit.  A cell depends on its two items alone: not on the launch geometry, not on the
 * other items of the call, not on how the item lists are split into calls.  n_a == 0, n_b == 0 or n_rows == 0 returns
 * WSAE_OK and touches nothing.  An active value of +inf, or a u that overflows, is the caller's duty to avoid: distances
 * of items that hold one are unspecified.  Workspace (8-byte aligned): wsae_dtw_workspace_bytes - that of
 * wsae_dyn_update, the canonical code of all n_rows.
 *
 * wsae_abx_count.  dist fp32 [n_x, ldd] holds rows x_lo .. x_lo + n_x - 1 of an items x items distance matrix (ldd >=
 * n_items, x_lo >= 0, x_lo + n_x <= n_items); cat, ctx, spk int32 [n_items] in device memory.  ctx is nullable (= one
 * context); spk is nullable only with WSAE_ABX_ANY, which ignores it.  An item takes part iff cat lies in [0, n_cats)
 * (1 <= n_cats <= WSAE_ABX_MAX_CATS), ctx >= 0 where ctx is given and spk >= 0 where the mode reads it.  An ordered
 * triple (a, b, x) of three distinct items that take part, x in the window, is admissible iff cat[a] == cat[x] != cat[b],
 * ctx[a] == ctx[b] == ctx[x], and under WSAE_ABX_WITHIN spk[a] == spk[b] == spk[x], under WSAE_ABX_ACROSS
 * spk[a] == spk[b] != spk[x].  An admissible triple whose dist[x][a] or dist[x][b] is NaN adds 1 to skipped[0].  Any
 * other adds 1 to total[cat[x]][cat[b]] and, to wins2[cat[x]][cat[b]], 2 where dist[x][a] < dist[x][b] and 1 where they
 * are equal.  wins2, total int64 [n_cats, n_cats] and skipped int64 [1]: caller-owned, zero-initialised device memory.
 * All sums are integers: windows, shards and call orders add, whatever the launch geometry.  n_x == 0 returns WSAE_OK and
 * touches nothing.  Workspace (8-byte aligned): wsae_abx_workspace_bytes - 4 bytes per (x, item): the a-candidates of a
 * row. */
#define WSAE_DTW_MAX_LEN 64
#define WSAE_DTW_MAX_K 128
#define WSAE_DTW_COSINE 0
#define WSAE_DTW_JACCARD 2 /* the numbering of WSAE_DYN_* */
#define WSAE_ABX_ANY 0
#define WSAE_ABX_WITHIN 1
#define WSAE_ABX_ACROSS 2
#define WSAE_ABX_MAX_CATS 1024
int64_t wsae_dtw_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_a, int32_t n_b);
int wsae_dtw_matrix(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg, const float* weight,
                    int64_t n_rows, const int32_t* a_start, const int32_t* a_len, int32_t n_a, const int32_t* b_start,
                    const int32_t* b_len, int32_t n_b, int32_t metric, int32_t normalize, float* dist, int32_t* steps,
                    int64_t ldd, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wsae_abx_workspace_bytes(int32_t n_items, int32_t n_x, int32_t n_cats);
int wsae_abx_count(const float* dist, int64_t ldd, int32_t x_lo, int32_t n_x, int32_t n_items, const int32_t* cat,
                   const int32_t* ctx, const int32_t* spk, int32_t n_cats, int32_t mode, int64_t* wins2, int64_t* total,
                   int64_t* skipped, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- token association: feature-by-token counts in a device hash table ------------------------------
 * The sparse counterpart of the label association: exact integer statistics of every (feature, token) pair that occurs,
 * for vocabularies of up to WSAE_PAIR_MAX_TOKENS tokens, in memory proportional to the number of distinct pairs, straight
 * from a compact code vals / idx [n_rows, k] (1 <= k <= WSAE_PAIR_MAX_K) and tokens int32 [n_rows].  Ctx-free; the caller's
 * stream, no allocation, no host synchronisation, no float atomics; argument errors are found on the host before any HIP
 * call.
 *
 * Activity (the rule of wsae_label_update): feature f is active on row r iff the row is not padding (seg[r] >= 0, or seg
 * == NULL) and some entry has idx == f, v > 0 and 0 <= f < hidden; an index repeated within a row counts once, with the
 * value of its first active entry.  NaN is never active, +inf is.  Pairs: with the call's single lag (-1024 <= lag <=
 * 1024) row r forms a pair iff it is not padding, 0 <= r + lag < n_rows, seg[r + lag] == seg[r] and 0 <= tokens[r + lag]
 * < n_tokens (1 <= n_tokens <= WSAE_PAIR_MAX_TOKENS); its token is t = tokens[r + lag].  Any other token value (-1 = "no
 * token") drops the pair and nothing else.  Lags never cross an utterance: a call sees whole utterances.
 *
 * State (caller-owned device memory).  The table: keys uint64 [cap], every slot initialised to 2^64 - 1 = empty; cnt
 * int32 [cap] and sum_q int64 [cap], zero-initialised; cap a power of two, 2^10 <= cap <= 2^31.  The key of a pair is
 * (uint64) f << 32 | t, which never reaches the empty marker.  status int64 [2], zero-initialised: {occupied slots,
 * dropped contributions}.  The marginals, zero-initialised: feat_rows int64 [hidden], tok_rows int64 [n_tokens],
 * pair_rows int64 [1].
 *
 * wsae_pair_update.  Per pair (r, t): pair_rows += 1, tok_rows[t] += 1, and for every feature f active on r with value v:
 * feat_rows[f] += 1 and, in the table under the key of (f, t), cnt += 1 and sum_q += rint(min(v, 4096) 2^20) (the fixed
 * point of wsae_profile_update).  Insertion: the first slot is h(key) & (cap - 1) with h the splitmix64 finaliser,
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 * in uint64 arithmetic; probing is linear with wrap-around; a probe reads the slot and, where it sees it empty, makes one
 * 64-bit compare-and-swap (empty -> key); a slot that was empty or holds the key takes the two integer adds.  Every slot
 * claimed adds 1 to status[0].  Nothing locks and nothing waits for another thread: the only loop is the probe loop, of at
 * most cap probes; a contribution that finds no slot within them adds 1 to status[1] and is dropped (the marginals still
 * count it).  The caller keeps status[0] before the call + n_rows k <= cap / 2: then nothing is ever dropped and probe
 * sequences stay short.  Every field is an integer sum: the set of (key, cnt, sum_q) triples and the marginals do not
 * depend on the launch geometry, on the order of the calls or on the grouping of whole utterances into calls; the slot a
 * key lands in may vary from run to run, and nothing reads the layout.  0 <= n_rows <= 2^31 - 1 per call; n_rows == 0
 * returns WSAE_OK and touches nothing.
 *
 * wsae_pair_merge.  Every slot of the source (src_keys / src_cnt / src_sum_q [src_cap], src_cap >= 1, any number - a
 * table or a plain list) whose key is not empty is inserted into the destination table by the rule above, with its cnt
 * and sum_q added; status is the destination's.  Serves growth (into an empty table of twice the size), the merge of two
 * shards and loading; the marginals are plain vectors that the caller adds.  The caller keeps status[0] + the occupied
 * slots of the source <= cap / 2.  The two tables must not be the same memory.
 *
 * wsae_pair_top.  by == WSAE_PAIR_BY_FEATURE: per feature (n_groups == hidden) over its tokens; by == WSAE_PAIR_BY_TOKEN:
 * per token (n_groups == n_tokens) over its features.  ids int32 [n_groups, n], scores fp64 [n_groups, n], counts int32
 * [n_groups, n], sums int64 [n_groups, n] (1 <= n <= WSAE_PAIR_MAX_N): per group the n pairs with the best score, sorted
 * by score descending, then id ascending (the id is the token of a feature's list and the feature of a token's); pairs
 * with cnt < min_count are skipped; the tail of a short list is (-1, -inf, 0, 0).  A key whose feature or token lies
 * outside [0, hidden) x [0, n_tokens) is skipped.  Scores are fp64 from the integers in exactly this operation order,
 * with c = cnt, a = feat_rows[f], b = tok_rows[t], N = pair_rows[0], each converted to double first:
 *     WSAE_PAIR_COUNT c;  WSAE_PAIR_PRECISION c / a;  WSAE_PAIR_RECALL c / b;  WSAE_PAIR_F1 (2 c) / (a + b);
 *     WSAE_PAIR_JACCARD c / ((a + b) - c);  WSAE_PAIR_LIFT (c N) / (a b);  WSAE_PAIR_MEAN ((double) sum_q 2^-20) / c
 * IEEE multiplies, adds and divides only, so a host loop reproduces every bit (a pair whose score is NaN - marginals that
 * do not belong to the table - is skipped).  The order is total, so the result does not depend on the slot layout.
 * Workspace (8-byte aligned): wsae_pair_top_workspace_bytes - two uint32 vectors over the groups and one over the slots;
 * -1 for invalid arguments; contents arbitrary on entry. */
#define WSAE_PAIR_MAX_K 128
#define WSAE_PAIR_MAX_TOKENS (1 << 24)
#define WSAE_PAIR_MAX_N 32
#define WSAE_PAIR_BY_FEATURE 0
#define WSAE_PAIR_BY_TOKEN 1
#define WSAE_PAIR_COUNT 0
#define WSAE_PAIR_PRECISION 1
#define WSAE_PAIR_RECALL 2
#define WSAE_PAIR_F1 3
#define WSAE_PAIR_JACCARD 4
#define WSAE_PAIR_LIFT 5
#define WSAE_PAIR_MEAN 6
int wsae_pair_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                     const int32_t* tokens, int64_t n_rows, int32_t n_tokens, int32_t lag, uint64_t* keys, int32_t* cnt,
                     int64_t* sum_q, int64_t cap, int64_t* status, int64_t* feat_rows, int64_t* tok_rows, int64_t* pair_rows,
                     void* stream);
int wsae_pair_merge(const uint64_t* src_keys, const int32_t* src_cnt, const int64_t* src_sum_q, int64_t src_cap, uint64_t* keys,
                    int32_t* cnt, int64_t* sum_q, int64_t cap, int64_t* status, void* stream);
int64_t wsae_pair_top_workspace_bytes(int64_t cap, int32_t n_groups);
int wsae_pair_top(const uint64_t* keys, const int32_t* cnt, const int64_t* sum_q, int64_t cap, const int64_t* feat_rows,
                  const int64_t* tok_rows, const int64_t* pair_rows, int32_t hidden, int32_t n_tokens, int32_t by,
                  int32_t n_groups, int32_t score, int32_t min_count, int32_t n, int32_t* ids, double* scores, int32_t* counts,
                  int64_t* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- token alignment: cross-attention cost and DTW to frame labels ---------------------------------
 * Whisper's word-timestamp recipe as two kernels: the attention weights of a few alignment heads are z-scored over the
 * token axis, median-filtered along time, averaged over the heads and negated (wsae_align_cost); dynamic time warping
 * over that tokens x frames matrix gives every encoder frame the token row that owns it (wsae_align_dtw).  Ctx-free; the
 * caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are found on the host before
 * any HIP call.  Every output of an utterance depends on that utterance alone: not on the launch geometry, not on the
 * other utterances of the call.  A sequential loop reproduces every bit (tests/align_oracle.py).
 *
 * wsae_align_cost.  w [n_utt, n_heads, ld_t, ld_f] of w_dtype WSAE_DT_F32, WSAE_DT_BF16 or WSAE_DT_F16 (every value converts
 * to double exactly); n_tok, n_frames int32 [n_utt] in DEVICE memory: the token rows and the encoder frames of utterance
 * u that are read (Whisper's num_frames // 2 crop); width odd, 1 <= width <= WSAE_ALIGN_MAX_WIDTH, p = width / 2;
 * 1 <= n_heads <= WSAE_ALIGN_MAX_HEADS.  An utterance is invalid iff n_tok < 1, n_tok > min(ld_t, WSAE_ALIGN_MAX_TOK),
 * n_frames <= p, n_frames > min(ld_f, WSAE_ALIGN_MAX_FRAMES), or any w[u][h][i < n_tok][j < n_frames] is not finite.
 * Nothing else of w is read.  For head h and frame j < n_frames:
 *   mean = (ONE chain of fp64 additions from 0 of double(w[h][i][j]), i = 0 .. n_tok - 1) / double(n_tok);
 *   var  = (ONE chain of fp64 additions from 0 of d d, d = double(w[h][i][j]) - mean: product, then add, no fused
 *          multiply-add) / double(n_tok) - the population variance; sd = sqrt(var) in fp64;
 *   z[h][i][j] = float((double(w[h][i][j]) - mean) / sd) + 0.0f (one rounding; never -0), and 0 where sd == 0;
 *   m[h][i][j] = the median of z[h][i][q] over q = j - p .. j + p, a q outside [0, n_frames) reflected (q -> -q,
 *          q -> 2 (n_frames - 1) - q: F.pad(mode = "reflect")) - a selection, so its bits are unique;
 *   cost[u][i][j] = float(0.0 - S / double(n_heads)), S = ONE chain of fp64 additions from 0 of double(m[h][i][j]) in head
 *          order.
 * cost fp32 [n_utt, ld_t, ld_f]: every element is written - rows >= n_tok, frames >= n_frames and invalid utterances as
 * WSAE_ALIGN_FILL (+inf).  n_bad int32 [n_utt]: 0 for a valid utterance, -1 where the sizes are invalid, else the number of
 * non-finite values among those read.  status int64 [2], caller-owned and zero-initialised: status[0] += the invalid
 * utterances, status[1] += the non-finite values (integer atomics).  z and m never exist in global memory.
 *
 * wsae_align_dtw.  cost fp32 [n_utt, ld_t, ld_f]; row_first, row_count, n_frames int32 [n_utt] in device memory: the
 * alignment runs over rows row_first .. row_first + row_count - 1 (n = row_count rows) and frames 0 .. n_frames - 1
 * (k frames) of cost[u] - the caller drops the start-of-transcript prefix and the end-of-text row this way.  n_bad is
 * nullable (that of wsae_align_cost).  An utterance is invalid iff n_bad[u] != 0, row_first < 0, n < 1,
 * n > WSAE_ALIGN_MAX_TOK, row_first + n > ld_t, k < 1, k > min(ld_f, WSAE_ALIGN_MAX_FRAMES), or a cost read is not
 * finite.  The recurrence is Whisper's, D in fp32: D[-1][-1] = 0, every other border +inf,
 *   D[i][j] = cost[i][j] + c (one fp32 addition), with c0 = D[i-1][j-1], c1 = D[i-1][j], c2 = D[i][j-1]:
 *   c = c0 (diagonal) if c0 < c1 and c0 < c2; else c = c1 (up) if c1 < c0 and c1 < c2; else c = c2 (left).
 * The path is walked back from (n - 1, k - 1) along the recorded choices; row 0 goes left, column 0 goes up.  Rows are
 * numbered as in cost (row_first + i):
 *   frame_pos int32 [n_utt, ld_f]: the largest row on the path at that frame (the row that starts there owns the frame,
 *     as in Whisper's jumps); -1 from n_frames on and for invalid utterances;
 *   tok_start int32 [n_utt, ld_t]: the first frame of every row on the path; tok_end: the start of the next row, n_frames
 *     for the last one (a zero-length token has start == end); both -1 outside the rows and for invalid utterances;
 *   path_cost fp32 [n_utt]: D[n-1][k-1] (WSAE_ALIGN_FILL where invalid); path_len int32 [n_utt]: the cells of the path (0
 *     where invalid);
 *   status int64 [2], zero-initialised: status[0] += the invalid utterances, status[1] += the non-finite costs read.
 * Workspace (8-byte aligned): wsae_align_workspace_bytes(n_utt, ld_t, ld_f) - two bits per cell, the recorded choices; -1
 * for invalid arguments; contents arbitrary on entry.  One workgroup per utterance; no wave waits for another anywhere but
 * at a workgroup barrier, and every loop is bounded by the sizes.  n_utt == 0 returns WSAE_OK and touches nothing. */
#define WSAE_DT_F16 2 /* wsae_align_cost only */
#define WSAE_ALIGN_MAX_TOK 512
#define WSAE_ALIGN_MAX_FRAMES 2048
#define WSAE_ALIGN_MAX_HEADS 32
#define WSAE_ALIGN_MAX_WIDTH 15
#define WSAE_ALIGN_FILL (__builtin_inff())
int wsae_align_cost(const void* w, int32_t w_dtype, int32_t n_utt, int32_t n_heads, int64_t ld_t, int64_t ld_f,
                    const int32_t* n_tok, const int32_t* n_frames, int32_t width, float* cost, int32_t* n_bad, int64_t* status,
                    void* stream);
int64_t wsae_align_workspace_bytes(int32_t n_utt, int64_t max_tok, int64_t max_frames);
int wsae_align_dtw(const float* cost, int32_t n_utt, int64_t ld_t, int64_t ld_f, const int32_t* row_first,
                   const int32_t* row_count, const int32_t* n_frames, const int32_t* n_bad, int32_t* frame_pos,
                   int32_t* tok_start, int32_t* tok_end, float* path_cost, int32_t* path_len, int64_t* status, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- log-mel front end: framing, windowed DFT, mel filter bank, log and clamp ----------------------
 * Waveforms in, Whisper's input_features out, as two kernels.  Ctx-free; the caller's stream, no allocation, no host
 * synchronisation, no float atomics; argument errors are found on the host before any HIP call.  Every output of an
 * utterance depends on that utterance alone, and every cell before the per-utterance clamp on its own frame alone: not on
 * the tile, the batch position or the launch geometry.  tests/logmel_oracle.py restates all of this in numpy.
 *
 * Constants (Whisper's, compile-time): n_fft = WSAE_LOGMEL_NFFT = 400, hop = WSAE_LOGMEL_HOP = 160, WSAE_LOGMEL_BINS = 201
 * frequency bins, n_mels 80 or 128.
 *
 * Batch.  x [n_utt] rows of stride ld_x (elements) of x_dtype WSAE_DT_F32 or WSAE_DT_I16 (int16 is scaled by 2^-15: exact);
 * length int32 [n_utt] in DEVICE memory: utterance u has len = min(max(length[u], 0), max_length) valid samples and is
 * zero from len to P = n_samples; nothing of x beyond len is read.  max_length (host) is the caller's bound on the lengths:
 * 0 <= max_length <= min(ld_x, P).  P is a multiple of 160, 480 <= P <= 2^28; T = P / 160 frames.
 *
 * Frame t covers q = 160 t .. 160 t + 399 of the length-P signal padded by 200 reflected samples at both ends
 * (np.pad(mode = "reflect") around P, not around length[u]): padded sample q is signal sample s = q - 200, with s < 0 -> -s
 * and s >= P -> 2 (P - 1) - s.  Frame T + 1 of torch.stft does not exist here.
 *
 * DFT.  basis fp32 [400][WSAE_LOGMEL_COLS = 416], 16-byte aligned, supplied by the caller: column k (k = 0 .. 200) is the
 * windowed cosine of bin k, column WSAE_LOGMEL_SIN_COL + k = 208 + k its sine; columns 201 .. 207 and 409 .. 415 are
 * padding and must be zero.  (The Python layer builds w[n] cos(2 pi ((k n) mod 400) / 400) in fp64 with the periodic Hann
 * window w and rounds once.)  The window lives in the table, the other operand is the raw sample:
 *   re[t][k] = ONE chain acc = fmaf(sample[160 t + n], basis[n][k], acc) from acc = 0 over n = 0, 1, .. 399 in this order
 * (v_mfma_f32_16x16x4_f32: bit for bit this chain); im[t][k] likewise with column 208 + k.
 * Power.  p[t][k] = fl(fl(re re) + fl(im im)): two fp32 products, one fp32 sum, no fused multiply-add.
 * Mel.  filt fp32 [201][n_mels] supplied by the caller;
 *   mel[t][m] = ONE chain acc = fmaf(p[t][k], filt[k][m], acc) from 0 over k = 0 .. 200 in this order.
 * Log.  v = log10f(mel) where mel > WSAE_LOGMEL_FLOOR = 1e-10f, else exactly -10 (log10(max(mel, 1e-10)); a NaN gives -10).
 * Tail, per utterance and in fp32, the extractor's order: M[u] = max of v over all n_mels x T cells;
 *   v = max(v, M[u] - 8); out = (v + 4) / 4.
 * out fp32 [n_utt][n_mels][T] with strides ld_u, ld_m, 1 (ld_m >= T, ld_u >= n_mels ld_m, ld_m <= 2^21): the layout the
 * encoder takes.  Only the cells (u, m, t < T) are written.  mel_power (nullable), same strides: mel[t][m] before floor and
 * log.  With out, mel_power 16-byte aligned and ld_m, ld_u multiples of 4 the stores are 16 bytes wide, and write-through
 * with 64-byte alignment and multiples of 16; any other alignment is served by 4-byte stores of the same values.
 * x and out are aligned to their elements (2 bytes for int16 x, else 4): anything else is WSAE_ERR_INVALID.
 * Workspace (4-byte aligned): wsae_logmel_workspace_bytes(n_utt, n_samples, n_mels) - one maximum per 64 frames; -1 for
 * invalid arguments; contents arbitrary on entry.  n_utt == 0 returns WSAE_OK and touches nothing. */
#define WSAE_DT_I16 3 /* wsae_logmel, wsae_clip_extract and wsae_resample only */
#define WSAE_LOGMEL_NFFT 400
#define WSAE_LOGMEL_HOP 160
#define WSAE_LOGMEL_BINS 201
#define WSAE_LOGMEL_COLS 416
#define WSAE_LOGMEL_SIN_COL 208
#define WSAE_LOGMEL_FLOOR 1e-10f
int64_t wsae_logmel_workspace_bytes(int32_t n_utt, int64_t n_samples, int32_t n_mels);
int wsae_logmel(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, const int32_t* length, int64_t max_length,
                int64_t n_samples, const float* basis, const float* filt, int32_t n_mels, float* out, int64_t ld_m, int64_t ld_u,
                float* mel_power, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- audio clip export: cut, peak, gain, fades and PCM conversion of many clips at once -------------
 * n_clips sample ranges of a device-resident bank of waveforms go to one output buffer, each at its own offset, as two
 * kernels.  Ctx-free; the caller's stream, no allocation, no host synchronisation, no float atomics; argument errors are
 * found on the host before any HIP call.  A clip's output depends on that clip's samples and table entries alone: not on
 * the other clips, their order, the tile or the alignment of either side.  tests/clip_oracle.py restates all of this in numpy.
 *
 * Bank.  x [n_utt] rows of stride ld_x (elements) of x_dtype WSAE_DT_F32 or WSAE_DT_I16 (int16 is scaled by 2^-15: exact);
 * length int32 [n_utt] in DEVICE memory: utterance u has L_u = min(max(length[u], 0), max_length) samples and nothing of x
 * at or beyond L_u is read.  max_length (host) is the caller's bound on the lengths, 0 <= max_length <= ld_x, below 2^31.
 * Samples must be finite.
 * Clip tables, all in DEVICE memory (a selection made on the device feeds the call without a host round trip):
 * clip_utt int32, clip_start int64, clip_count int32, clip_off int64, each [n_clips].  max_count (host, 0 .. 2^30) bounds the
 * counts - it sizes the grid and the workspace - and a larger count is clamped to it; a negative count is 0.
 * Bounds of clip c: u = clip_utt[c]; s0 = max(clip_start[c], 0); e = min(s0 + count, L_u); n = max(e - s0, 0).  A negative
 * start moves to 0 and keeps its count; the end is cut at the length (the reference's extract_clip).
 * Peak.  m = max_j |x_j| over the n samples, float32 (0 for an empty clip).
 * Arithmetic, float32, no fused multiply-add, IEEE division:
 *   gain_mode WSAE_CLIP_GAIN_PEAK and m > 0: y_j = fl(fl(x_j / m) * target);  otherwise y_j = x_j.
 *   fade = F >= 1: y_j = fl(y_j * r_j), r_j = fl(float(min(min(j, n - 1 - j) + 1, F)) / float(F));  F = 0: no fade.
 * Output at out[clip_off[c] + j], j < n.  out_dtype WSAE_DT_F32: y_j.  WSAE_DT_I16: clamp(rintf(fl(y_j * 32767)), -32768,
 * 32767) - round half to even.  The one exception: GAIN_NONE, F = 0, int16 in and int16 out copies the samples unchanged.
 * out_len int32 [n_clips]: n, or -1 for an invalid clip - u outside [0, n_utt), clip_off[c] < 0 or clip_off[c] + n >
 * out_elems - of which no sample is written.  out_peak float32 [n_clips], nullable: m (0 for an invalid clip).
 * Only the n cells of a clip are written, gaps between clips stay untouched, so one call serves the padded
 * [n_clips][ld] layout and a montage with silences between the clips.  Output ranges must not overlap (the caller's
 * contract).  x and out are aligned to their element size; any clip_start and clip_off are served: the bulk of a clip leaves
 * as 16-byte stores from the first 64-byte boundary of its output on, write-through, the ends elementwise, same values.
 * Workspace (4-byte aligned): wsae_clip_workspace_bytes(n_clips, max_count) - one float per clip and WSAE_CLIP_TILE
 * samples of max_count, at least one per clip; -1 for invalid arguments; contents arbitrary on entry.  n_clips == 0 returns
 * WSAE_OK and touches nothing. */
#define WSAE_CLIP_TILE 4096 /* samples per workgroup */
#define WSAE_CLIP_GAIN_NONE 0
#define WSAE_CLIP_GAIN_PEAK 1
int64_t wsae_clip_workspace_bytes(int32_t n_clips, int64_t max_count);
int wsae_clip_extract(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, const int32_t* length, int64_t max_length,
                      int32_t n_clips, const int32_t* clip_utt, const int64_t* clip_start, const int32_t* clip_count,
                      int64_t max_count, const int64_t* clip_off, int32_t gain_mode, float target, int32_t fade, void* out,
                      int32_t out_dtype, int64_t out_elems, int32_t* out_len, float* out_peak, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- resampling: downmix, polyphase FIR, lengths and PCM conversion ---------------------------------
 * Interleaved waveforms at one rate in, mono waveforms at another out, as one kernel.  Ctx-free; the caller's stream, no
 * allocation, no host synchronisation, no atomics, no workspace; argument errors are found on the host before any HIP call.
 * An utterance's output depends on that utterance's samples and the tables alone: not on its row, the other rows, the tile
 * or the alignment of either side.  tests/resample_oracle.py restates all of this in numpy.
 *
 * Input.  x [n_utt] rows of stride ld_x (elements) of x_dtype WSAE_DT_F32 or WSAE_DT_I16 (int16 is scaled by 2^-15: exact).
 * Frames are interleaved: sample m of channel c of utterance u is x[u ld_x + m channels + c] (what `wave` and `soundfile`
 * give); 1 <= channels <= WSAE_RESAMPLE_MAX_CHANNELS = 8.  length int32 [n_utt] in DEVICE memory, counted in frames:
 * L_u = min(max(length[u], 0), max_length), and nothing of x at or beyond frame L_u is read.  max_length (host) bounds the
 * lengths: 0 <= max_length < 2^31, max_length channels <= ld_x.  Samples must be finite.
 * Downmix, float32, once, before the filter: channels == 1: mono[m] = x[m].  Otherwise s = x[m][0]; s = fl(s + x[m][c]) for
 * c = 1 .. channels - 1 in this order; mono[m] = fl(s / float(channels)), an IEEE division.
 * Filter.  orig and new_ (the two rates divided by their gcd) lie in 1 .. WSAE_RESAMPLE_MAX_RATE = 1024 and are coprime.
 * taps fp32 [new_][n_taps] row-major and first int32 [new_], both in device memory; 1 <= n_taps <= WSAE_RESAMPLE_MAX_TAPS =
 * 512.  halo (host, 0 .. WSAE_RESAMPLE_MAX_HALO = 4096, n_taps <= orig + 2 halo) is the caller's promise that -halo <=
 * first[p] and first[p] + n_taps <= orig + halo for every p; a first[p] that breaks it is clamped into that range, so that no
 * access leaves the staged span, and the values of that phase are then unspecified.  With xz[m] = mono[m] for 0 <= m < L_u
 * and 0 elsewhere, and j = i new_ + p (0 <= p < new_):
 *   y[j] = ONE chain acc = fmaf(xz[i orig + first[p] + w], taps[p][w], acc) from acc = +0 over w = 0, 1, .. n_taps - 1 in
 * this order; padding taps (zeros) take part like any other.
 * Lengths.  out_len int32 [n_utt] in device memory: ceil(new_ L_u / orig), computed in int64 (torchaudio's target_length).
 * Every cell j < out_cols (host) of a row is written: y[j] for j < out_len[u], zero for the rest; cells at or beyond
 * out_cols and anything behind the last row stay untouched.  ceil(new_ max_length / orig) <= out_cols <= ld_y, out_cols < 2^31.
 * Output.  out [n_utt] rows of stride ld_y (elements).  out_dtype WSAE_DT_F32: y[j].  WSAE_DT_I16: clamp(rintf(fl(y[j] *
 * 32768)), -32768, 32767), round half to even - the inverse of the scaling on the way in (NOT the 32767 of the clip writer,
 * which follows the WAV convention).  x and out are aligned to their elements; any ld_x, ld_y and base are served: the bulk
 * of a row's tile leaves as 16-byte stores from its first 64-byte boundary on, write-through, the ends elementwise, same
 * values; mono and stereo rows whose frames meet the 16-byte boundaries are read 16 bytes wide, all others by element.
 * Identity.  orig = new_ = 1, taps = [[1.0f]], first = [0], halo = 0: fmaf(x, 1, +0) = x for every finite x up to the sign of
 * a zero; the downmix and both conversions are still served.
 * Geometry.  A workgroup owns WSAE_RESAMPLE_TILE consecutive outputs of an utterance and holds their input span, the
 * tap table and the converted outputs in at most WSAE_RESAMPLE_LDS_BYTES of LDS; the tile is halved until the span fits, and
 * a table that does not fit beside it is read through the cache.  (Within the limits above one block always fits.)
 * n_utt == 0 returns WSAE_OK and touches nothing. */
#define WSAE_RESAMPLE_TILE 1024 /* outputs per workgroup */
#define WSAE_RESAMPLE_LDS_BYTES 65536
#define WSAE_RESAMPLE_MAX_CHANNELS 8
#define WSAE_RESAMPLE_MAX_RATE 1024
#define WSAE_RESAMPLE_MAX_TAPS 512
#define WSAE_RESAMPLE_MAX_HALO 4096
int wsae_resample(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, int32_t channels, const int32_t* length,
                  int64_t max_length, int32_t orig, int32_t new_, const float* taps, const int32_t* first, int32_t n_taps,
                  int32_t halo, void* out, int32_t out_dtype, int64_t ld_y, int64_t out_cols, int32_t* out_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WSAE_H_ */
