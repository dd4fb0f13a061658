/*
 * unitspeech_hip.h -- C ABI of the MI355X-native UnitSpeech diffusion decoder (libunitspeech_hip.so).
 *
 * The reference has no plugin/FFI layer: its hot path sits behind the Python class API of
 * `unitspeech/unitspeech.py`.  Each entry point below names the reference method it
 * replaces.  Conventions: every function returns 0 on success or a negative US_E* code and never throws;
 * all tensor pointers are DEVICE pointers to contiguous fp32 unless marked "host"; the caller owns every
 * buffer; work is enqueued on the given hipStream_t and the library does not synchronise; a handle is bound
 * to the device that was current at creation and is not thread-safe.
 */
#ifndef UNITSPEECH_HIP_H
#define UNITSPEECH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct us_decoder* us_handle;
typedef void* us_stream;              /* hipStream_t */

enum {
  US_OK = 0,
  US_EINVAL = -1,      /* bad argument / unsupported shape */
  US_ENOKEY = -2,      /* unknown state_dict key */
  US_ESHAPE = -3,      /* tensor shape does not match the configured architecture */
  US_EWEIGHTS = -4,    /* forward called before every weight was loaded */
  US_EWORKSPACE = -5,  /* workspace too small */
  US_EHIP = -6         /* a HIP runtime call failed (see us_last_error) */
};

/* Constructor arguments of `UnitSpeech.__init__` (unitspeech/unitspeech.py:221) /
 * `GradLogPEstimator2d.__init__` (:125).  heads=4, dim_head=32, groups=8 are fixed by the reference
 * (:79, :47).  dim must be a multiple of 16; n_mults <= 6. */
typedef struct us_config {
  int32_t n_feats;      /* 80 */
  int32_t dim;          /* 128 */
  int32_t n_mults;      /* 4 */
  int32_t dim_mults[6]; /* 1,2,4,8 */
  int32_t spk_emb_dim;  /* 256 */
  float beta_min;       /* 0.05 */
  float beta_max;       /* 20.0 */
  float pe_scale;       /* 1000 */
} us_config;

/* UnitSpeech(...) constructor.  Allocates the packed device weight store (not the weights' values). */
int us_decoder_create(us_handle* out, const us_config* cfg);
/* The same with creation flags.  US_CREATE_EXACT_FP32: every GEMM of this handle runs on the exact-fp32 matrix instruction
 * (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain) instead of the f16x3 form (three fp16 MFMA products of two-plane split operands,
 * fp32-accurate for operands inside the fp16 range): the path for tensors beyond +-65504, see us_range_status. */
enum { US_CREATE_EXACT_FP32 = 1 };
int us_decoder_create_ex(us_handle* out, const us_config* cfg, unsigned flags);
int us_decoder_destroy(us_handle h);

/* f16x3 operand range.  The reference computes in plain fp32 (unitspeech/unitspeech.py:46-96); the default handle forms its GEMM
 * products from fp16 planes, which represent |x| < 65520.  A larger operand is never clamped: it becomes an infinity (the affected
 * outputs are non-finite, as loud as an overflow can be; a NaN input stays a NaN, as in the reference) and the split that met it
 * ORs a bit into a per-handle device word: US_RANGE_ACT for an activation, Winograd-domain value or gradient, US_RANGE_WEIGHT for a
 * weight at load time (or a folded attention weight).  us_range_status copies the word to *status (0 = every result since the last
 * reset is fp32-accurate), optionally clears it, and WAITS for `stream`; the _async form only enqueues the copy into the caller's
 * (pinned) host word.  A caller that sees a non-zero status repeats the call on a US_CREATE_EXACT_FP32 handle -- the Python mirror
 * does so by itself (unitspeech_amd/unitspeech.py: _Engine.range_status, UnitSpeech._run_checked). */
enum { US_RANGE_ACT = 1, US_RANGE_WEIGHT = 2 };
int us_range_status(us_handle h, unsigned* status, int reset, us_stream stream);
int us_range_status_async(us_handle h, unsigned* status_host, int reset, us_stream stream);

/* `load_state_dict` for one tensor: `key` is the reference state_dict key (e.g.
 * "estimator.downs.0.0.block1.block.0.weight"), `data` a device pointer in the reference's own layout
 * (Conv2d OIHW, ConvTranspose2d IOHW, Linear [out,in]).  The library repacks into its MFMA-friendly layout
 * on `stream`.  Re-loading a key (fine-tuning) is allowed. */
int us_decoder_load_weight(us_handle h, const char* key, const float* data, const int64_t* shape, int ndim,
                           us_stream stream);
/* Completes a batch of us_decoder_load_weight calls: tensors the library keeps in the reference's own layout (biases,
 * GroupNorm affine, MLP weights, the unconditional embeddings) are copied, and the split-precision packs of the convolution
 * weights are written, by ONE table-driven launch each, enqueued here: every `data` pointer handed to us_decoder_load_weight
 * must stay valid until this call has been made on the same stream.  Every computing entry point refuses to run (US_EWEIGHTS)
 * while loads are pending. */
int us_decoder_flush_weights(us_handle h, us_stream stream);
/* Training mode of the weight store.  Inference runs the stride-1 3x3 convolutions of the low-resolution levels as Winograd F(4x4,3x3) /
 * F(2x4,3x3) where enabled (US_WINO4; csrc/wino4.hip), from a third pack of those weights (36 / 24 matrices per convolution) that the
 * training path never reads.  training != 0: us_decoder_load_weight skips that pack -- an optimiser step re-loads every tensor -- and
 * marks it stale; inference calls then run the F(2x2,3x3) form for such a tensor (correct, slower, rounding of that form) until it is
 * loaded again with training == 0.  us_decoder_stale_inference_forms: how many loaded tensors are in that state (a host mirror
 * re-loads them before its first inference call after training: unitspeech_amd/unitspeech.py, _Engine.sync_weights). */
int us_decoder_set_training(us_handle h, int training);
int us_decoder_stale_inference_forms(us_handle h);
/* Number of state_dict tensors the configured architecture has / that have been loaded so far. */
int us_decoder_num_weights(us_handle h);
int us_decoder_num_loaded(us_handle h);
/* Name of the i-th expected key (state_dict order); NULL when out of range. */
const char* us_decoder_weight_key(us_handle h, int i);

/* Scratch bytes needed by one us_estimator_forward call on Bp items of T frames. */
size_t us_workspace_bytes(us_handle h, int Bp, int T);
/* Scratch bytes needed by us_reverse_diffusion for a micro-batch of `mb` utterances (n_cfg branches each). */
size_t us_sampler_workspace_bytes(us_handle h, int mb, int T, int n_cfg);

/* `GradLogPEstimator2d.forward(x, mask, mu, t, spk_emb)` (unitspeech/unitspeech.py:164-201).
 * x, mu, out: [Bp, n_feats, T]; mask: [Bp, 1, T] (0/1); t: [Bp]; spk: [Bp, 1, spk_emb_dim].  T % 2^(n_mults-1) == 0. */
int us_estimator_forward(us_handle h, const float* x, const float* mask, const float* mu, const float* t,
                         const float* spk, float* out, int Bp, int T, void* workspace, size_t workspace_bytes,
                         us_stream stream);

/* `UnitSpeech.forward` == `reverse_diffusion(z, mask, cond, spk_emb, n_timesteps, text_gradient_scale,
 * spk_gradient_scale)` (unitspeech/unitspeech.py:333-391), for any B with per-item B=1 semantics.
 * z, cond, out: [B, n_feats, T]; mask: [B,1,T]; spk: [B,1,spk_emb_dim].
 * noise: [N, B, n_feats, T] explicit gaussian draws replacing `torch.randn` at :367, or NULL to use the
 *        built-in counter-based generator keyed by (seed, utterance index + utt_offset, step).
 * coef_host: optional HOST table [N][8] of per-step scalars (see us_step_coefficients); NULL = computed
 *        by the library.
 * micro_batch: utterances processed together (0 = library default); workspace must hold
 *        us_sampler_workspace_bytes(h, min(micro_batch, B), T, n_cfg).
 * mel_range_host: NULL, or HOST {mel_min, mel_max}: the caller's next step, the mel de-normalisation
 *        `(y + 1) / 2 * (mel_max - mel_min) + mel_min` (inference.py:140) that feeds the vocoder, is applied in the
 *        sampler's last pass (same fp32 operation order), so `out` is the vocoder's input [B, n_feats, T]. */
int us_reverse_diffusion(us_handle h, const float* z, const float* mask, const float* cond, const float* spk,
                         const float* noise, uint64_t seed, int64_t utt_offset, int B, int T, int n_timesteps,
                         float text_gradient_scale, float spk_gradient_scale, const float* coef_host,
                         int micro_batch, const float* mel_range_host, float* out, void* workspace, size_t workspace_bytes,
                         us_stream stream);

/* Host helper: the per-step scalars the sampler update consumes, [N][8] fp32:
 * {sqrt_recip_acp, sqrt_recipm1_acp*sqrt_1m_acp, sqrt(acp_prev), sqrt(1-acp_prev-sigma^2), sqrt_1m_acp,
 *  [idx!=0]*sigma, t_i, 0} for i = 0..N-1 (`register_beta` :235-271, `p_mean_variance` :273-296). */
int us_step_coefficients(int n_timesteps, float beta_min, float beta_max, float* coef_host);

/* Fill out[n] with N(0,1) draws of the built-in generator (Philox4x32-10 + Box-Muller), stream (seed, key). */
int us_fill_normal(float* out, size_t n, uint64_t seed, uint64_t key, us_stream stream);

/* FLOPs (2*MAC of conv + attention einsums + MLPs) of one estimator evaluation per item. */
double us_estimator_flops(us_handle h, int T);

/* ---- training (fine-tune) path: `loss_t` forward + `loss.backward()` through the score network -------------------
 * us_estimator_forward_train == us_estimator_forward, but every tensor the backward needs is kept inside `workspace`
 * (sized by us_train_workspace_bytes), which must stay untouched until us_estimator_backward has been enqueued or the
 * tape has been released.  *tape_id names this forward's record; several may be live at once (each in its own
 * workspace; beyond 16 the oldest is dropped).
 * us_estimator_backward(tape_id, grad_out [B, n_feats, T]) writes d loss / d parameter for every `estimator.*` state_dict
 * key into the caller's buffers (reference layout and shape of that key; overwritten, not accumulated).  keys[i]/grads[i]
 * pair a key with its device buffer; all estimator keys must be present.  B, T must be the forward's.  Fails with
 * US_EINVAL when tape_id is not live (consumed, released or evicted) -- a backward never runs on another forward's tape.
 * grad_x, grad_mu [B, n_feats, T], grad_spk [B, spk_emb_dim]: optional (NULL = not wanted) gradients w.r.t. the inputs
 * x, mu and spk_emb (the reference's trainers reach the text / unit encoder through them: train_STEP1.py:381,
 * train_STEP2.py:299).  The tape is consumed by the call (unless US_BACKWARD_KEEP_TAPE, below).  Outside a stream capture the call
 * runs the weight-gradient launches on a second stream of the handle, fenced against `stream` by events on both sides: when it
 * returns, everything it enqueued is ordered before whatever the caller enqueues on `stream` next (US_WGRAD_STREAM=0: one stream). */
size_t us_train_workspace_bytes(us_handle h, int B, int T);
int us_estimator_forward_train(us_handle h, const float* x, const float* mask, const float* mu, const float* t,
                               const float* spk, float* out, int B, int T, void* workspace, size_t workspace_bytes,
                               uint64_t* tape_id, us_stream stream);
/* flags: US_BACKWARD_GRADS_ZEROED (bit 0) = the gradient buffers are already zero (e.g. views of one zero-filled blob): skips 228
 * fill launches.  US_BACKWARD_KEEP_TAPE (bit 1) = the tape stays live after a successful call: for a caller that re-runs the SAME forward
 * launches into the SAME workspace itself (a captured HIP graph of the forward, replayed per iteration) and then calls the backward
 * again -- the record names buffers, not values.  Release it with us_tape_release.
 * Range of grad_out: any.  The backward GEMMs split their fp32 operands into two fp16 planes, which carry full
 * precision from about 6e-5 upwards, while the gradient of a mean-reduced loss over B*F*T elements is ~1/(B*F*T) and a caller's loss
 * weight or accumulation factor comes on top: the entry point itself multiplies grad_out by the power of two that brings its largest
 * magnitude to [2^-7, 2^-6) (chosen on the device from the data), runs the pass, and multiplies everything it returns by the inverse
 * -- exact, because the pass is linear in grad_out.  grad_out is not modified. */
enum { US_BACKWARD_GRADS_ZEROED = 1, US_BACKWARD_KEEP_TAPE = 2 };
int us_estimator_backward(us_handle h, uint64_t tape_id, const float* grad_out, int B, int T, const char* const* keys,
                          float* const* grads, int n_grads, int flags, float* grad_x, float* grad_mu, float* grad_spk,
                          us_stream stream);
/* Drop a tape whose backward will never run (its workspace may then be reused). */
int us_tape_release(us_handle h, uint64_t tape_id);
/* 1 when us_estimator_backward OVERWRITES every element of this key's gradient buffer (the convolution weights: 99.9 % of the gradient
 * bytes), so the buffer needs no zero-fill under US_BACKWARD_GRADS_ZEROED; 0 when the backward accumulates into it; -1: unknown key. */
int us_grad_is_overwritten(us_handle h, const char* key);

/* ---- elementwise steps of the training objective (no handle) -------------------------------------------------------
 * `forward_diffusion(x0, mask, t)` (unitspeech/unitspeech.py:376-384) with the gaussian draw z passed in:
 *   xt = (x0 * exp(-c/2) + z * sqrt(1 - exp(-c))) * mask, z_masked = z * mask, c = beta_min*t + (beta_max-beta_min)/2*t^2.
 *   z == NULL: xt = x0 * exp(-c/2) * mask only (the backward of xt w.r.t. x0, applied to a gradient).
 * `loss_t`'s objective (:403-404): loss[0] = sum((score * sqrt(1 - exp(-c)) + z_masked)^2) / (sum(mask) * F); dscore
 *   (optional) = d loss / d score.  scratch: us_diffusion_loss_scratch_bytes(B, F, T) bytes. */
int us_forward_diffusion(const float* x0, const float* mask, const float* t, const float* z, float* xt, float* z_masked,
                         int B, int F, int T, float beta_min, float beta_max, us_stream stream);
size_t us_diffusion_loss_scratch_bytes(int B, int F, int T);
int us_diffusion_loss(const float* score, const float* z_masked, const float* t, const float* mask, float* loss,
                      float* dscore, int B, int F, int T, float beta_min, float beta_max, void* scratch,
                      size_t scratch_bytes, us_stream stream);
/* out[i] = x[i] * scalar_dev[0] (chain rule with a device-resident upstream gradient); out = x * mask[b][t] on [B,F,T]. */
int us_scale(const float* x, const float* scalar_dev, float* out, size_t n, us_stream stream);
int us_mul_mask(const float* x, const float* mask, float* out, int B, int F, int T, us_stream stream);
/* scale_and_inverse[0] = 2^k with max|x| * 2^k in [2^(target_log2 - 1), 2^target_log2), [1] = 2^-k (device floats; 1, 1 for an all-zero
 * or non-finite x): an exact, data-driven scaling factor (what us_estimator_backward applies to its grad_out internally); feed [0] and
 * [1] to us_scale. */
int us_pow2_scale(const float* x, size_t n, int target_log2, float* scale_and_inverse, us_stream stream);
/* `fine_tune`'s segment crop (:458-486).  cond_x [B,F,Lu], y [B,F,Ly], attn [B,Lu,Ly]; start/count: DEVICE int64 [B]
 * (crop offset and number of valid frames min(y_length, segment_size) per item).  Writes y_cut, cond_y [B,F,segment_size]
 * (cond_y = attn_cut^T cond_x, masked) and seg_mask [B,segment_size]. */
int us_finetune_segment(const float* cond_x, const float* y, const float* attn, const int64_t* start, const int64_t* count,
                        float* y_cut, float* cond_y, float* seg_mask, int B, int F, int Lu, int Ly, int segment_size,
                        us_stream stream);
/* Transpose of us_finetune_segment's alignment (the unit-encoder step, train_STEP2.py:295-297): d_cond_x [B,F,Lu] =
 * attn_cut d_cond_y, i.e. d_cond_x[b][f][l] = sum_{j < count[b]} attn[b][l][start[b] + j] d_cond_y[b][f][j].  Overwrites d_cond_x. */
int us_finetune_segment_backward(const float* d_cond_y, const float* attn, const int64_t* start, const int64_t* count, float* d_cond_x, int B,
                                 int F, int Lu, int Ly, int segment_size, us_stream stream);
/* Prior loss of train_STEP2.py:302-303: loss[0] (device) = sum(0.5 ((y - mu_y)^2 + log 2 pi) y_mask) / (sum(y_mask) F) over y, mu_y
 * [B,F,T], y_mask [B,1,T]; d_mu_y (optional) = its gradient w.r.t. mu_y.  One workgroup, fixed summation order: no scratch. */
int us_prior_loss(const float* y, const float* mu_y, const float* y_mask, float* loss, float* d_mu_y, int B, int F, int T, us_stream stream);

/* ---- text-to-speech training step (train_STEP1.py:307-387), csrc/tts_train.hip ------------------------------------------
 * us_mas_log_prior: the log-prior of monotonic alignment search (:336-342) times maximum_path's mask: log_prior [B,Tx,Ty] =
 *   (-0.5 sum_f y^2 + sum_f mu_x y - 0.5 sum_f mu_x^2 - 0.5 F log 2 pi) x_mask[b][x] y_mask[b][y] for mu_x [B,F,Tx], y [B,F,Ty],
 *   x_mask [B,1,Tx], y_mask [B,1,Ty]; masked cells are 0.
 * us_maximum_path: glow-tts `maximum_path` (:343) over log_prior [B,Tx,Ty] with tx = x_lengths[b], ty = y_lengths[b] (device,
 *   int64, clamped to [0, Tx] / [0, Ty]): attn [B,Tx,Ty] fp32 0/1 (overwritten), durations [B,Tx] = row sums of attn.  The path is
 *   bit-identical to the sequential algorithm (fp32 accumulation, -1e9 sentinels, strict comparison in the backtrack), also for
 *   tx > ty.  Tx <= 1024.  The per-item decision table lives in LDS when it fits (Tx * ceil(Ty / 32) words, 512 x 2048 does);
 *   otherwise the caller passes us_maximum_path_workspace_bytes of device scratch (0 when every item fits).  No host sync.
 * us_duration_loss: loss[0] (device) = sum((logw - log(1e-8 + durations) x_mask)^2) / sum(x_lengths) over logw, x_mask [B,1,Tx],
 *   durations [B,Tx] (:348-349); d_logw (optional) = its gradient w.r.t. logw.  One workgroup, fixed summation order. */
int us_mas_log_prior(const float* mu_x, const float* y, const float* x_mask, const float* y_mask, float* log_prior, int B, int F, int Tx,
                     int Ty, us_stream stream);
size_t us_maximum_path_workspace_bytes(int B, int Tx, int Ty);
int us_maximum_path(const float* log_prior, const int64_t* x_lengths, const int64_t* y_lengths, float* attn, float* durations, int B, int Tx,
                    int Ty, void* workspace, size_t workspace_bytes, us_stream stream);
int us_duration_loss(const float* logw, const float* durations, const float* x_mask, const int64_t* x_lengths, float* loss, float* d_logw,
                     int B, int Tx, us_stream stream);

/* ---- conditioning producer of `execute_text_to_speech` (:424-438; the text encoder and duration predictor stay the
 * caller's modules) -----------------------------------------------------------------------------------------------------
 * us_tts_durations: w_ceil[B,L] = ceil(exp(logw) * x_mask) * length_scale, y_lengths[B] (int64) = max(sum_l w_ceil, 1).
 * us_tts_align: `generate_path` (unitspeech/util.py:27-40) + `attn^T cond_x` + `sequence_mask`: cond_y [B,F,Tp] (frame t
 *   takes the column of the symbol whose duration interval contains t; zeros at t >= y_lengths[b]), y_mask [B,Tp]
 *   (optional), attn [B,L,Tp] 0/1 (optional).  cond_x [B,F,L]. */
int us_tts_durations(const float* logw, const float* x_mask, float* w_ceil, int64_t* y_lengths, int B, int L,
                     float length_scale, us_stream stream);
int us_tts_align(const float* cond_x, const float* w_ceil, const float* x_mask, const int64_t* y_lengths, float* cond_y,
                 float* attn, float* y_mask, int B, int F, int L, int Tp, us_stream stream);
/* ---- mel-rate alignment of voice conversion (scripts/voice_conversion.py:22-33), the counterpart of us_tts_align --------
 * us_vc_align: cond_y [B,F,Tp] = F.interpolate(cond_x[b, :, :x_lengths[b]], size=y_lengths[b], mode='linear') per item, each as
 *   if it were alone (never from the padded L), zeros on [y_lengths[b], Tp); y_mask [B,Tp] = t < y_lengths[b].  cond_x [B,F,L];
 *   x_lengths, y_lengths [B] int64 on the device, which the caller has validated: 1 <= x_lengths[b] <= L, 1 <= y_lengths[b] <= Tp
 *   (values outside are clamped, so nothing is read out of bounds).  The source coordinate is evaluated exactly in integers:
 *   num = max((2t + 1) Lx - Ly, 0), i0 = num / (2 Ly), lambda = (num mod 2 Ly) / (2 Ly), out = (1 - lambda) x[i0] + lambda x[i1].
 *   One launch, no host sync. */
int us_vc_align(const float* cond_x, const int64_t* x_lengths, const int64_t* y_lengths, float* cond_y, float* y_mask, int B, int F,
                int L, int Tp, us_stream stream);

/* ---- the two learned modules of the conditioning producer, inference -------------------------------
 * `Encoder` (unitspeech/encoder.py:253-308; text encoder and unit encoder are two instances) and `DurationPredictor`
 * (unitspeech/duration_predictor.py:24-63, reverse=True).  Same conventions as the decoder handle: the caller owns the
 * activation scratch (us_frontend_workspace_bytes), nothing is allocated or freed by a forward call, and a call made while
 * another device than the handle's is current is refused (US_EINVAL).  Dropout is the identity (eval mode).  `n_contentvec > 0`
 * (encoder.py:279-283: a Linear(n_contentvec -> n_channels, bias=False) instead of the Embedding; checkpoints/voice-conversion.json
 * sets 768) is a handle kind of its own, us_encoder_create_contentvec below; `heads_share=False` is not built -- no
 * configuration of the reference uses it (conf/hydra_config.py:85-116). */
typedef struct us_frontend* us_frontend_handle;
typedef struct us_encoder_config {
  int32_t n_vocab;          /* len(symbols) + 1 (text) / n_units (unit encoder) */
  int32_t n_feats;          /* 80 */
  int32_t n_channels;       /* 192 */
  int32_t filter_channels;  /* 768 */
  int32_t n_heads;          /* 2 */
  int32_t n_layers;         /* 6 */
  int32_t kernel_size;      /* 3 (FFN convolutions; the prenet's 3 layers of kernel 5 are fixed, encoder.py:283) */
  int32_t window_size;      /* 4; 0 = no relative-position terms (window_size=None) */
} us_encoder_config;
typedef struct us_duration_config {
  int32_t in_channels;      /* 192 */
  int32_t filter_channels;  /* 256 */
  int32_t kernel_size;      /* 3 */
  int32_t spk_emb_dim;      /* 256; 0 = no speaker conditioning (g = None) */
} us_duration_config;
int us_encoder_create(us_frontend_handle* out, const us_encoder_config* cfg);
int us_duration_predictor_create(us_frontend_handle* out, const us_duration_config* cfg);
int us_frontend_destroy(us_frontend_handle h);
/* `load_state_dict` for one tensor, reference key and layout (Conv1d [out,in,k], Embedding [vocab,channels], emb_rel_* [1,2W+1,D]). */
int us_frontend_load_weight(us_frontend_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_frontend_num_weights(us_frontend_handle h);
const char* us_frontend_weight_key(us_frontend_handle h, int i);
const char* us_frontend_last_error(us_frontend_handle h);
/* `Encoder.forward(x, x_lengths)` (:294-308): ids [B,L] int64, lengths [B] int64 (device) ->
 * mu_x [B,n_feats,L], x [B,n_channels,L], x_mask [B,1,L]. */
size_t us_frontend_workspace_bytes(us_frontend_handle h, int B, int L);
int us_encoder_forward(us_frontend_handle h, const int64_t* ids, const int64_t* lengths, float* mu_x, float* x, float* x_mask, int B, int L,
                       void* workspace, size_t workspace_bytes, us_stream stream);
/* The Encoder with a Linear front (the ContentVec encoder of voice conversion).  us_encoder_create_contentvec: cfg as for
 * us_encoder_create (cfg->n_vocab is ignored), 1 <= n_contentvec <= 1024 else US_EINVAL; the key table is the reference's, with
 * emb.weight [n_channels, n_contentvec] (Linear layout) and every other key unchanged.
 * us_encoder_forward_features: feats [B,L,n_contentvec] fp32 in place of the ids; outputs and workspace as us_encoder_forward.
 *   x0 = (feats . emb.weight^T) * sqrt(n_channels) runs on the fp32 matrix cores, reduction order fixed and independent of B and L;
 *   rows at or past lengths[b] are NOT READ (they may hold anything, NaN included) and give zeros.  The convolutions run on the
 *   fp32 FMA kernel of us_encoder_forward (measured faster than the matrix-core GEMM at L = 499 and 1499).  An id handle here, or a
 *   ContentVec handle in us_encoder_forward / us_encoder_forward_train / us_encoder_backward, is US_EINVAL.
 * us_encoder_forward_features_train / us_encoder_backward_features: us_encoder_forward_train / us_encoder_backward for such a
 *   handle (same schedule, tape, workspace size, dropout sites and gradient table).  The backward takes feats again (the tape does
 *   not copy them) and produces emb.weight's gradient [n_channels, n_contentvec] = sqrt(n_channels) * sum over valid rows of
 *   dx0[row][c] * feats[row][k] with the split weight-gradient GEMM, partial sums added in a fixed order; there is no gradient
 *   with respect to feats. */
int us_encoder_create_contentvec(us_frontend_handle* out, const us_encoder_config* cfg, int32_t n_contentvec);
int us_encoder_forward_features(us_frontend_handle h, const float* feats, const int64_t* lengths, float* mu_x, float* x, float* x_mask,
                                int B, int L, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_forward_features_train(us_frontend_handle h, const float* feats, const int64_t* lengths, float* mu_x, float* x,
                                      float* x_mask, int B, int L, float p_dropout, uint64_t seed, void* workspace,
                                      size_t workspace_bytes, us_stream stream);
int us_encoder_backward_features(us_frontend_handle h, const float* feats, const float* grad_mu, const float* grad_x, int B, int L,
                                 const char* const* keys, float* const* grads, int n_grads, void* workspace, size_t workspace_bytes,
                                 us_stream stream);
/* ---- training of the Encoder (encoder.py:253-308 in train mode; csrc/encoder_train.hip) --------------------------------
 * us_encoder_forward_train: the forward with every Dropout of the reference -- the prenet's three relu_drop (p = 0.5), and in
 *   each transformer layer the attention probabilities, EncoderModule.drop after attention, the FFN's drop after the ReLU and
 *   EncoderModule.drop after the FFN (p = p_dropout, 0 <= p_dropout < 1).  p_dropout < 0: no site drops, the prenet's
 *   included (the reference in eval mode, through which autograd still runs).  Same inputs and outputs as us_encoder_forward.  The
 *   workspace (us_encoder_train_workspace_bytes) keeps the tape the backward reads; it must stay untouched until then.  The
 *   tape stores every activation (about 7 C + F floats per symbol and layer) and the attention probabilities (B H L^2 floats
 *   per layer; stored rather than recomputed), plus the backward's scratch and a gradient slot for every key.
 * us_encoder_backward: overwrites grads[i] (reference layout of keys[i], device memory) with the gradient of that state_dict
 *   key, given upstream gradients grad_mu [B,n_feats,L] and / or grad_x [B,n_channels,L] (either may be NULL: zero).  Keys not
 *   listed are computed into the workspace and dropped.  US_EINVAL when the workspace holds no training forward of this B and L.
 *   Deterministic: no atomics, fixed summation orders.
 * Dropout masks are a pure function of (seed, site, flat index of the element in the reference's tensor): Philox4x32-10 keyed by
 *   the seed, counter (index / 4, site).  Sites: 0, 1, 2 the prenet layers ([B,C,L]); for transformer layer i, 3 + 4i the attention
 *   probabilities ([B,H,L,L]), 4 + 4i the drop after attention ([B,C,L]), 5 + 4i the FFN's drop ([B,filter_channels,L]), 6 + 4i the
 *   drop after the FFN ([B,C,L]).
 * us_encoder_dropout_mask: TEST HOOK.  Writes the scaled keep mask (0 or 1 / (1 - p)) that `site` used for `seed` in a training
 *   forward with this p_dropout, in the shape listed above: p = 0.5 at the prenet sites and p_dropout elsewhere (all ones for a
 *   negative p_dropout).  A pure function of its arguments.
 * us_encoder_tape_release: forget the training forward a workspace holds (call before the memory is freed or reused); a later
 *   us_encoder_backward on it fails with US_EINVAL. */
size_t us_encoder_train_workspace_bytes(us_frontend_handle h, int B, int L);
int us_encoder_forward_train(us_frontend_handle h, const int64_t* ids, const int64_t* lengths, float* mu_x, float* x, float* x_mask, int B,
                             int L, float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_backward(us_frontend_handle h, const float* grad_mu, const float* grad_x, int B, int L, const char* const* keys,
                        float* const* grads, int n_grads, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_dropout_mask(us_frontend_handle h, uint64_t seed, int site, int B, int L, float p_dropout, float* out, us_stream stream);
int us_encoder_tape_release(us_frontend_handle h, const void* workspace);
/* TEST HOOKS: one launch group of the Encoder's training forward / backward alone, through the host function the forward or the
 * backward calls, for kernel-level parity tests (tests/test_encoder_train_kernels_gpu.py).  Activations are channel-last
 * [B][L][C] (row = b * L + l), as the kernels see them; mask is [B][L].  All work goes on `stream`; scratch is the caller's
 * workspace of us_encoder_debug_workspace_bytes(h, B, L) bytes (one size serves every hook); nothing is allocated.  A bad
 * argument is US_EINVAL and an unknown key or layer US_ENOKEY, both before any launch; every weight must be loaded.
 * us_encoder_debug_conv: the Conv1d `key` ("prenet.conv_layers.0", "encoder.ffn_layers.1.conv_2", "proj_m", ...), Cout x Cin x K.
 *   US_ENCODER_CONV_FWD:   out [B][L][Cout] = (add + drop(relu(conv(in [* mask]) + bias))) [* mask]: in [B][L][Cin]; the flags pick
 *     the input mask, the ReLU and the output mask; add [B][L][Cout] or NULL; drop_site >= 0 applies that site's keep mask for
 *     (seed, p_dropout) (us_encoder_dropout_mask with the same p; the site's channel count must be Cout), < 0 none.
 *   US_ENCODER_CONV_WGRAD: dw [Cout][Cin][K] (torch layout) and db [Cout] from in [B][L][Cin] (read times mask with MASK_IN) and
 *     the output gradient dout [B][L][Cout].
 *   US_ENCODER_CONV_DGRAD: out [B][L][Cin] = (add + dgrad(dout)) [gate > 0 ? * gate_scale : 0] [* mask]: gate [B][L][Cin] or NULL.
 *   Operands a mode does not take must be NULL / 0.
 * us_encoder_debug_ln_bwd: backward of the LayerNorm `key` ("prenet.norm_layers.0", "encoder.norm_layers_1.2", ...) over
 *   n_channels: x (its input), dy, and optionally gate with gate_scale (dy is first taken as gate > 0 ? dy * gate_scale : 0: the
 *   prenet's ReLU and dropout) -> dx [B][L][C], dgamma [C], dbeta [C].
 * us_encoder_debug_attention: the attention of transformer layer `layer` in its training form on the caller's q, k, v [B][L][C]:
 *   out [B][L][C] and P [B][H][L][L] (the probabilities before dropout); the keep mask is that of site 3 + 4 * layer for
 *   (seed, p_dropout), p_dropout in [0, 1).  With dO [B][L][C] also the backward: DS [B][H][L][L], dq, dk, dv [B][L][C] and the
 *   gradients of emb_rel_k / emb_rel_v [2W+1][D] (NULL when window_size is 0); without dO all of these are NULL.
 * us_encoder_debug_embed_grad: grad [n_vocab][C] of emb.weight from ids [B][L] and the gradient dx0 [B][L][C] of emb(ids) * sqrt(C). */
enum { US_ENCODER_CONV_FWD = 0, US_ENCODER_CONV_WGRAD = 1, US_ENCODER_CONV_DGRAD = 2 };
enum { US_ENCODER_CONV_MASK_IN = 1, US_ENCODER_CONV_RELU = 2, US_ENCODER_CONV_MASK_OUT = 4 };
size_t us_encoder_debug_workspace_bytes(us_frontend_handle h, int B, int L);
int us_encoder_debug_conv(us_frontend_handle h, const char* key, int mode, const float* in, const float* dout, const float* mask,
                          const float* add, const float* gate, float gate_scale, unsigned flags, int drop_site, float p_dropout, uint64_t seed,
                          float* out, float* dw, float* db, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_debug_ln_bwd(us_frontend_handle h, const char* key, const float* x, const float* dy, const float* gate, float gate_scale,
                            float* dx, float* dgamma, float* dbeta, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_debug_attention(us_frontend_handle h, int layer, const float* q, const float* k, const float* v, const float* mask, float p_dropout,
                               uint64_t seed, float* out, float* P, const float* dO, float* DS, float* dq, float* dk, float* dv,
                               float* grad_rel_k, float* grad_rel_v, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream);
int us_encoder_debug_embed_grad(us_frontend_handle h, const int64_t* ids, const float* dx0, float* grad, int B, int L, us_stream stream);
/* `DurationPredictor.forward(x, x_mask, w=None, g=g, reverse=True)` (:47-63): x [B,in_channels,L], x_mask [B,1,L],
 * g [B,1,spk_emb_dim] (NULL iff spk_emb_dim == 0) -> logw [B,1,L]. */
int us_duration_predictor_forward(us_frontend_handle h, const float* x, const float* x_mask, const float* g, float* logw, int B, int L,
                                  void* workspace, size_t workspace_bytes, us_stream stream);
/* ---- training of the DurationPredictor (duration_predictor.py:47-63 in train mode; csrc/duration_train.hip) -----------------
 * The Encoder's training ABI, one for one, on a duration-predictor handle.
 * us_duration_predictor_forward_train: same inputs and output as us_duration_predictor_forward, with the reference's two Dropouts
 *   (0 <= p_dropout < 1; 0 draws nothing; p_dropout < 0: the reference in eval mode, differentiated).  The workspace
 *   (us_duration_predictor_train_workspace_bytes) keeps the tape the backward reads -- the concatenated input, the mask and the two
 *   convolutions' outputs after the ReLU -- plus the backward's scratch and a gradient slot for every key; it must stay untouched
 *   until then.
 * us_duration_predictor_backward: overwrites grads[i] (reference layout of keys[i], device memory) with the gradient of that
 *   state_dict key, given grad_logw [B,1,L].  All ten keys are available; keys not listed are computed into the workspace and
 *   dropped.  There is NO gradient for x (the reference detaches it, :48) and NONE for g: conv_1's data gradient is never computed.
 *   US_EINVAL when the workspace holds no training forward of this B and L (never run, released, or another handle's).
 *   Deterministic: no atomics, fixed summation orders.
 * Dropout masks are the Encoder's stream (Philox4x32-10 keyed by the seed, counter (index / 4, site)): site 0 follows norm_1,
 *   site 1 follows norm_2, flat index of the reference's [B,filter_channels,L] tensor.
 * us_duration_predictor_dropout_mask: TEST HOOK.  The scaled keep mask (0 or 1 / (1 - p)) [B,filter_channels,L] that `site` used
 *   for `seed` (all ones for p_dropout <= 0).  A pure function of its arguments.
 * us_duration_predictor_tape_release: forget the training forward a workspace holds (call before the memory is freed or reused).
 * us_duration_predictor_mse_loss: the reverse=False branch (:60-62) on its own: loss[0] = sum((logw - log(w + 1e-6) x_mask)^2) /
 *   sum(x_mask) and, when d_logw is not NULL, d loss / d logw [B,1,L]; logw, w, x_mask [B,1,L].  (us_duration_loss is train_STEP1's
 *   other statement: epsilon 1e-8 inside the log, divided by sum(x_lengths).) */
size_t us_duration_predictor_train_workspace_bytes(us_frontend_handle h, int B, int L);
int us_duration_predictor_forward_train(us_frontend_handle h, const float* x, const float* x_mask, const float* g, float* logw, int B, int L,
                                        float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes, us_stream stream);
int us_duration_predictor_backward(us_frontend_handle h, const float* grad_logw, int B, int L, const char* const* keys, float* const* grads,
                                   int n_grads, void* workspace, size_t workspace_bytes, us_stream stream);
int us_duration_predictor_dropout_mask(us_frontend_handle h, uint64_t seed, int site, int B, int L, float p_dropout, float* out,
                                       us_stream stream);
int us_duration_predictor_tape_release(us_frontend_handle h, const void* workspace);
int us_duration_predictor_mse_loss(const float* logw, const float* w, const float* x_mask, float* loss, float* d_logw, int B, int L,
                                   us_stream stream);

/* ---- one building block of the score network on its own (parity tests against per-module reference outputs) ---------
 * prefix: the module's state_dict prefix ("estimator.downs.1.1", "estimator.downs.1.2", "estimator.downs.1.3",
 * "estimator.ups.1.3"); level: resolution level whose geometry (n_feats >> level) x (T >> level) the block runs at.
 * x / out: pixel-major [B][H][W][C] (the library's internal activation layout), x already multiplied by the frame mask
 * where the reference masks the operand; mask: full-resolution [B][T]; temb: [B][dim + spk_emb_dim] (ResnetBlock only).
 * Output masking follows the library's producer-side convention (attention / Downsample / Upsample outputs are stored
 * masked): pass an all-ones mask to obtain the reference module's raw output.
 * US_DEBUG_TEMB (prefix ignored): x = t [B], out [B][2 * dim] = SinusoidalPosEmb(t) | mlp(SinusoidalPosEmb(t))
 * (unitspeech/unitspeech.py:109-121, 133-134, 165-166).
 * US_DEBUG_FIRST (prefix and level ignored): the first ResnetBlock, "estimator.downs.0.0", by the walk's own helper: x = mu [B][F][T]
 * followed by the noisy input [B][F][T] (both are multiplied by the mask here, as the walk stacks them), temb as above;
 * out [B][F][T][dim], stored masked.
 * US_DEBUG_FINAL (prefix ignored): the final Block and the 1x1 projection (unitspeech/unitspeech.py:198-201): x [B][F][T][dim] already
 * masked, out [B][F][T] (masked).  level selects where the Block's activation lives: 0 = not kept, GroupNorm + Mish run inside the
 * projection (every inference evaluation); 1 = kept, the projection in its plain form (what a training forward runs). */
enum { US_DEBUG_BLOCK = 0, US_DEBUG_RESNET = 1, US_DEBUG_ATTENTION = 2, US_DEBUG_DOWN = 3, US_DEBUG_UP = 4, US_DEBUG_TEMB = 5,
       US_DEBUG_FIRST = 6, US_DEBUG_FINAL = 7 };
int us_debug_block(us_handle h, int kind, const char* prefix, int level, const float* x, const float* mask,
                   const float* temb, float* out, int B, int T, void* workspace, size_t workspace_bytes, us_stream stream);

/* Sampled kernel timing for the roofline report.  When enabled, the middle evaluation of every
 * us_reverse_diffusion micro-batch (and every us_estimator_forward) brackets each implicit-GEMM convolution launch,
 * and the evaluation as a whole, with HIP events on the caller's stream.  us_profile_read waits for the recorded
 * events and returns the accumulated totals: time and algorithmic FLOPs (2*MAC) of the conv launches, their
 * count, and the time / count of the sampled evaluations. */
int us_profile_enable(us_handle h, int enable);
int us_profile_read(us_handle h, double* conv_ms, double* conv_flops, int64_t* conv_launches, double* eval_ms,
                    int64_t* evals, int reset);
/* The share of those conv launches that ran as f16x3 GEMMs (three fp16 MFMA products of two-plane split operands at fp32
 * accuracy): their time, their fp32-equivalent FLOPs (2*M*N*K; the fp16 matrix cores execute three times that) and their
 * count, as accumulated by the last us_profile_read (call it first, with reset = 0). */
int us_profile_read_f16(us_handle h, double* f16_ms, double* f16_flops, int64_t* f16_launches);

/* Gradient clipping + Adam over all parameter tensors in three launches.  Replaces torch.nn.utils.clip_grad_norm_(params, max_norm)
 * followed by torch.optim.Adam(lr, betas, eps, weight_decay=0).step()  (reference finetune.py:163-165, train_STEP1.py).
 *   p, g, m, v  device arrays [n_tensors] of device pointers: parameter, gradient, exp_avg, exp_avg_sq (fp32, same numel)
 *   numel       device [n_tensors]
 *   blk_tensor, blk_off  device [n_blocks]: block i works on elements [blk_off[i], blk_off[i] + 4096) of tensor blk_tensor[i]
 *   lr, beta1, beta2, eps  python-double hyper-parameters; 1 - beta, lr / (1 - beta1^step), sqrt(1 - beta2^step) are evaluated
 *               in double and rounded to fp32 once, as torch.optim.Adam's scalar arguments are
 *   step        1-based Adam step
 *   max_norm    > 0: total L2 norm over all gradients, g *= min(1, max_norm / (norm + 1e-6)) in place first; <= 0: no clipping
 *   partial     device scratch, n_blocks + 2 floats; on return partial[n_blocks] = total norm, partial[n_blocks+1] = coefficient
 * Enqueues on `stream`, never synchronises. */
int us_clip_adam_step(void* const* p, void* const* g, void* const* m, void* const* v, const int64_t* numel,
                      const int32_t* blk_tensor, const int64_t* blk_off, int n_tensors, int n_blocks, double lr, double beta1,
                      double beta2, double eps, int step, float max_norm, float* partial, us_stream stream);

/* ---- BigVGAN vocoder (unitspeech/vocoder/models.py:117-191, inference) -----------------------------------------------------
 * mel [B][num_mels][T] -> waveform [B][1][T * prod(upsample_rates)], exact fp32.  Same conventions as the front-end handles: weights
 * are loaded one state_dict tensor at a time from DEVICE memory, in the reference's key names of the remove_weight_norm() form
 * (weight norm folded by the caller), the caller owns the activation scratch (us_vocoder_workspace_bytes),
 * a forward call allocates nothing and only enqueues on `stream` (graph-capturable), and a call made while another device than the
 * handle's is current is refused (US_EINVAL).  Activation1d's two 12-tap filters are the state_dict buffers
 * `<act>.upsample.filter` / `<act>.downsample.lowpass.filter` [1, 1, 12], taken as given.  resblock "2" (AMPBlock2), up-samplers
 * whose kernel is not a multiple of their rate (or with kernel - rate odd) and rates above 16 are not built: us_vocoder_create
 * returns US_EINVAL for them. */
typedef struct us_vocoder* us_vocoder_handle;
enum { US_VOCODER_SNAKE = 0, US_VOCODER_SNAKEBETA = 1 };
typedef struct us_vocoder_config {
  int32_t num_mels;                      /* 80 */
  int32_t upsample_initial_channel;      /* 1536 (22 kHz / 80-band), 512 (base) */
  int32_t resblock;                      /* 1 = AMPBlock1 (2 is refused) */
  int32_t n_up;                          /* len(upsample_rates), <= 8 */
  int32_t upsample_rates[8];
  int32_t upsample_kernel_sizes[8];
  int32_t n_kernels;                     /* len(resblock_kernel_sizes), <= 4 */
  int32_t resblock_kernel_sizes[4];      /* odd */
  int32_t resblock_dilation_sizes[4][3];
  int32_t activation;                    /* US_VOCODER_SNAKE / US_VOCODER_SNAKEBETA */
  int32_t snake_logscale;                /* 1: alpha / beta are stored as logarithms */
} us_vocoder_config;
int us_vocoder_create(us_vocoder_handle* out, const us_vocoder_config* cfg);
int us_vocoder_destroy(us_vocoder_handle h);
int us_vocoder_load_weight(us_vocoder_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_vocoder_num_weights(us_vocoder_handle h);
const char* us_vocoder_weight_key(us_vocoder_handle h, int i);
const char* us_vocoder_last_error(us_vocoder_handle h);
size_t us_vocoder_workspace_bytes(us_vocoder_handle h, int B, int T);
/* `BigVGAN.forward(mel)` (:169-191): mel [B][num_mels][T] -> wav [B][1][T * prod(upsample_rates)]. */
int us_vocoder_forward(us_vocoder_handle h, const float* mel, float* wav, int B, int T, void* workspace, size_t workspace_bytes,
                       us_stream stream);
/* The same on a ragged batch: mel [B][num_mels][Tmax], of which item b is valid on its first lengths[b] frames; `lengths` is a HOST
 * array of B values in [1, Tmax] (null or a value outside that range: US_EINVAL naming the item, before anything is enqueued).  wav
 * [B][1][Tmax * hop]: item b's first lengths[b] * hop samples have exactly the bits us_vocoder_forward gives for that item alone at
 * T = lengths[b], and the samples past them are 0.0f.  Nothing at or past an item's end is read: the mel there and the whole workspace
 * may hold anything, NaN included.  Workspace: us_vocoder_workspace_bytes(h, B, Tmax).  Allocates nothing, copies nothing, only enqueues
 * (the lengths travel as kernel arguments, 32 items per launch), and B is not bound by us_vocoder_forward's B * channels <= 65535. */
int us_vocoder_forward_lengths(us_vocoder_handle h, const float* mel, const int64_t* lengths, float* wav, int B, int Tmax,
                               void* workspace, size_t workspace_bytes, us_stream stream);
/* One layer of the vocoder on its own, through the launch the forward uses (layer-level parity tests).  prefix names
 *  - a convolution: "conv_pre", "ups.<i>.0", "resblocks.<n>.convs1.<l>", "resblocks.<n>.convs2.<l>": in [B][Cin][Tin] -> out
 *    [B][Cout][Tin * rate] (rate 1 for a Conv1d) = conv(in) + bias, then + res, then sum + that, then / div, each only when given
 *    (res, sum null and div 0 otherwise; res and sum are [B][Cout][Tout] and either may be `out` itself, as in the forward);
 *  - an Activation1d: "resblocks.<n>.activations.<a>", "activation_post": in, out [B][C][Tin];
 *  - "conv_post": in [B][C][Tin] -> out [B][1][Tin], tanh included.
 * res, sum and div are refused (US_EINVAL) for the last two kinds; an unknown prefix is US_ENOKEY; us_vocoder_forward's size limits
 * apply to the layer's own tensors.  Needs every weight loaded; takes no workspace. */
int us_vocoder_debug_layer(us_vocoder_handle h, const char* prefix, const float* in, const float* res, const float* sum, float div, float* out,
                           int B, int Tin, us_stream stream);
/* us_vocoder_debug_layer on a ragged batch, through the launches us_vocoder_forward_lengths uses: rows are Tin_max (Tin_max * rate for
 * the output of an up-sampler) apart and item b has lengths[b] input steps (HOST array, B values in [1, Tin_max]).  A convolution or an
 * Activation1d leaves `out` untouched at and past an item's end; "conv_post" writes 0.0f there. */
int us_vocoder_debug_layer_lengths(us_vocoder_handle h, const char* prefix, const float* in, const float* res, const float* sum, float div,
                                   float* out, int B, int Tin_max, const int64_t* lengths, us_stream stream);

/* ---- ECAPA-TDNN speaker encoder (unitspeech/speaker_encoder/ecapa_tdnn.py:164-287, eval mode) --------------------------------
 * The upstream model's hidden states [L][B][T][feat_dim] -> embedding [B][emb_dim]: the softmax(feature_weight)-weighted sum of the L
 * hidden states, InstanceNorm1d, the ECAPA-TDNN trunk (k = 5 convolution, three SE-Res2 blocks with dilations 2 / 3 / 4, the 1536-channel
 * 1x1 convolution, attentive statistics pooling, BatchNorm1d, Linear) and, on request, the division by the norm (finetune.py:110).  fp32
 * storage and accumulation, exact fp32 products.  The upstream model itself (WavLM / HuBERT) and the fbank / mfcc extraction are not
 * part of the library.  Same conventions as the vocoder handle: weights are loaded one state_dict tensor at a time from DEVICE memory
 * in the reference's key names (every floating-point key except `feature_extract.*`; BatchNorm runs from its running statistics), the
 * caller owns the activation scratch (us_speaker_workspace_bytes), a forward call allocates nothing and only enqueues on `stream`, and
 * a call made while another device than the handle's is current is refused (US_EINVAL).  Every reduction has a fixed order: repeated
 * calls, and batch items alone or together, give the same bits.  SE_Res2Block shortcuts (in_channels != out_channels) do not occur in
 * the reference's configuration and are refused (US_ENOKEY for a `.shortcut.` key); channels must be a multiple of 8, at most 512. */
typedef struct us_speaker* us_speaker_handle;
typedef struct us_speaker_config {
  int32_t feat_dim;                      /* 1024 (WavLM-large hidden size) */
  int32_t channels;                      /* 512 */
  int32_t emb_dim;                       /* 256 */
  int32_t n_layers;                      /* length of feature_weight: 25 for WavLM-large; 0 = no feature_weight (fbank / mfcc form) */
  int32_t global_context_att;            /* 0 / 1: AttentiveStatsPool's global context */
} us_speaker_config;
enum { US_SPEAKER_STAGE_FEAT = 0, US_SPEAKER_STAGE_LAYER1 = 1, US_SPEAKER_STAGE_BLOCKS = 2, US_SPEAKER_STAGE_POOLING = 3 };
int us_speaker_create(us_speaker_handle* out, const us_speaker_config* cfg);
int us_speaker_destroy(us_speaker_handle h);
int us_speaker_load_weight(us_speaker_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_speaker_num_weights(us_speaker_handle h);
const char* us_speaker_weight_key(us_speaker_handle h, int i);
const char* us_speaker_last_error(us_speaker_handle h);
size_t us_speaker_workspace_bytes(us_speaker_handle h, int B, int T);
/* `ECAPA_TDNN.forward` from get_feat's input on (:261-287).  hidden_states is [L][B][T][feat_dim] with L = n_layers, or, with L = 0, the
 * already combined [B][feat_dim][T] (which only gets the InstanceNorm1d).  Any T >= 1; every item of the batch has T steps (the
 * reference has no masking; us_speaker_forward_lengths is the call for items of different lengths).  emb_out [B][emb_dim]; normalize = 1
 * divides the whole output by its norm (B = 1 only), 0 returns the raw output. */
int us_speaker_forward(us_speaker_handle h, const float* hidden_states, int L, int B, int T, float* emb_out, int normalize, void* workspace,
                       size_t workspace_bytes, us_stream stream);
/* The same forward on a ragged batch: hidden_states is [L][B][Tmax][feat_dim] (or, with L = 0, [B][feat_dim][Tmax]) and item b is valid on
 * its first lengths[b] steps.  `lengths` is a HOST array of B values in [1, Tmax]; they travel to the kernels as arguments, 32 items per
 * launch group, so the call still allocates nothing, copies nothing and only enqueues on `stream`.  Nothing at or past an item's end is
 * read into any result (it may hold anything, NaN included): the instance norm, the SE means, the global context and the attentive pooling
 * run over lengths[b] steps, the dilated convolutions see zeros past the end as they do past T, and row b of emb_out has exactly the bits
 * us_speaker_forward gives for that item alone at T = lengths[b].  normalize = 1 divides each row by its own norm (any B).  The
 * workspace is us_speaker_workspace_bytes(h, B, Tmax); afterwards us_speaker_stage(B, Tmax) shows [B][C][Tmax] tensors of which only each
 * item's first lengths[b] steps are defined.  A null `lengths`, or a lengths[b] outside [1, Tmax] (the message names b), is US_EINVAL
 * before anything is enqueued. */
int us_speaker_forward_lengths(us_speaker_handle h, const float* hidden_states, int L, int B, int Tmax, const int64_t* lengths, float* emb_out,
                               int normalize, void* workspace, size_t workspace_bytes, us_stream stream);
/* Debug view of an intermediate the last us_speaker_forward(B, T) or us_speaker_forward_lengths(B, Tmax) left in `workspace`: *data points into it, shape[3] is its extent.
 * FEAT [B][feat_dim][T] after get_feat, LAYER1 [B][channels][T], BLOCKS [B][3 channels][T] (layer2 | layer3 | layer4 along the
 * channels, the input of `conv`), POOLING [B][3072][1] (mean | std, before `bn`).  Enqueues nothing. */
int us_speaker_stage(us_speaker_handle h, int stage, int B, int T, void* workspace, size_t workspace_bytes, const float** data, int64_t* shape);
/* One dense convolution of the speaker encoder on its own, through the launch the forward uses (layer-level parity tests).  prefix:
 * "layer1.conv", "layer<l>.Conv1dReluBn<1|2>.conv", "conv", "pooling.linear1" (which reads the first 1536 of its weight's input
 * channels), "pooling.linear2".  out[b][co][t] = bn(act(conv(in)[b][co][t] + bias[co] + bias2[b][co])): act one of US_SPEAKER_ACT_*;
 * bias2 [B][Cout] or null; bn_prefix null or "" for none, else a BatchNorm the forward folds ("layer1.bn", "layer<l>.Conv1dReluBn<1|2>.bn",
 * "bn") with at least Cout channels, of which the first Cout are applied as one scale and one shift.  in / out are [B][C][T] with
 * in_bs / out_bs floats between batch items (>= C * T), so either may be a channel slice of a wider tensor.  An unknown prefix or
 * bn_prefix is US_ENOKEY.  Needs every weight loaded; takes no workspace. */
enum { US_SPEAKER_ACT_NONE = 0, US_SPEAKER_ACT_RELU = 1, US_SPEAKER_ACT_TANH = 2 };
int us_speaker_debug_conv(us_speaker_handle h, const char* prefix, const char* bn_prefix, int act, const float* in, int64_t in_bs, float* out,
                          int64_t out_bs, const float* bias2, int B, int T, us_stream stream);

/* ---- mel-spectrogram front end (unitspeech/vocoder/meldataset.py:51-74 with center=False; finetune.py:104), csrc/mel.hip --------
 * Waveform [B][Tmax] -> log-mel [B][num_mels][Tmax / hop]: reflect padding by (n_fft - hop) / 2, the windowed DFT as a convolution
 * with n_fft / hop taps over the de-interleaved waveform, sqrt(re^2 + im^2 + 1e-9), the mel projection, log(max(x, 1e-5)) and,
 * on request, the normalisation (m - mel_min) / (mel_max - mel_min) * 2 - 1 with every operation rounded on its own.  fp32 storage and
 * accumulation, exact fp32 products on the matrix cores.  Same conventions as the vocoder handle: the two weights are loaded from
 * DEVICE memory and taken as given, "mel_basis" [num_mels][n_fft / 2 + 1] (the filter bank) and "window" [win] (centred in n_fft
 * samples when shorter, as torch.stft does); loading mel_basis synchronises the stream once (the host learns how many bins have a
 * non-zero column: only those are computed).  The caller owns the scratch (us_mel_workspace_bytes); us_mel_forward and us_mel_minmax
 * allocate nothing and only enqueue on `stream` (graph-capturable: lengths are read on the host during the call), and a call made
 * while another device than the handle's is current is refused (US_EINVAL).  An item's frames depend on its own samples only and every
 * sum has a fixed order: an item alone or in a batch, and repeated calls, give the same bits.
 * us_mel_create returns US_EINVAL when hop does not divide n_fft, n_fft - hop is odd, win > n_fft or n_fft > 4096. */
typedef struct us_mel* us_mel_handle;
typedef struct us_mel_config {
  int32_t n_fft;                         /* 1024 */
  int32_t hop;                           /* 256 */
  int32_t win;                           /* 1024 */
  int32_t num_mels;                      /* 80 */
} us_mel_config;
int us_mel_create(us_mel_handle* out, const us_mel_config* cfg);
int us_mel_destroy(us_mel_handle h);
int us_mel_load_weight(us_mel_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_mel_num_weights(us_mel_handle h);
const char* us_mel_weight_key(us_mel_handle h, int i);
const char* us_mel_last_error(us_mel_handle h);
/* frames of a waveform of T samples: T / hop */
int us_mel_frames(us_mel_handle h, int T);
size_t us_mel_workspace_bytes(us_mel_handle h, int B, int Tmax);
/* wav [B][Tmax] (device); lengths: HOST int64 [B], the samples of each item, or NULL for Tmax each.  A length must be above
 * (n_fft - hop) / 2 (the reflection needs it) and at most Tmax, else US_EINVAL; samples at or past an item's length are never read.
 * mel_min / mel_max: device, n_norm values each with n_norm = 0 (no normalisation; both may be NULL), 1 (one range for all bands) or
 * num_mels (one per band).  out [B][num_mels][Tmax / hop]: item b has lengths[b] / hop frames, the ones past them are pad_value. */
int us_mel_forward(us_mel_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, const float* mel_min, const float* mel_max,
                   int n_norm, float pad_value, float* out, void* workspace, size_t workspace_bytes, us_stream stream);
/* out[0][m] = min, out[1][m] = max of mel[b][m][t] over b < B, t < lengths_frames[b] (HOST int64 [B] in [0, F], or NULL for F each):
 * the inner loop of preprocessing/process_mel_normalization.py.  mel [B][num_mels][F] and out [2][num_mels] on the device.  Exact in
 * any order; a NaN is skipped (fminf / fmaxf); +inf / -inf when there is no valid frame. */
int us_mel_minmax(us_mel_handle h, const float* mel, const int64_t* lengths_frames, int B, int F, float* out, us_stream stream);

/* ---- sinc resampler (torchaudio.transforms.Resample, as called at finetune.py:113 and data.py:75,193), csrc/resample.hip ----------
 * Waveform [B][Tmax] -> [B][us_resample_out_length(h, Tmax)].  With orig_freq and new_freq the two rates divided by their gcd and
 * K = orig_freq + 2 width, output sample i = q * new_freq + c of an item of len samples is
 *   out[i] = sum_{k < K} kernel[c][0][k] * y[q * orig_freq + k - width],  y = 0 outside [0, len),  i < ceil(new_freq * len / orig_freq):
 * torchaudio's strided convolution with its buffer "kernel" [new_freq][1][K], the one weight, loaded from DEVICE memory and taken as
 * given.  fp32 storage and accumulation, exact fp32 products on the matrix cores, the K products of an output added in sample order.
 * Same conventions as the mel handle: the caller owns the scratch (us_resample_workspace_bytes); us_resample_forward allocates nothing
 * and only enqueues on `stream` (lengths are read on the host during the call), a call made while another device than the handle's is
 * current is refused (US_EINVAL), and an item alone or in a batch, and repeated calls, give the same bits.
 * us_resample_create touches no device and returns US_EINVAL for a non-positive rate, rates with a common divisor, a rate above 4096,
 * a negative width or a width above 2^16.  (The fields are not called `orig` and `new`: the latter is a C++ keyword.) */
typedef struct us_resample* us_resample_handle;
typedef struct us_resample_config {
  int32_t orig_freq;                     /* 441 for 22050 -> 16000 */
  int32_t new_freq;                      /* 320 */
  int32_t width;                         /* 9: ceil(lowpass_filter_width * orig_freq / (rolloff * min(orig_freq, new_freq))) */
} us_resample_config;
int us_resample_create(us_resample_handle* out, const us_resample_config* cfg);
int us_resample_destroy(us_resample_handle h);
int us_resample_load_weight(us_resample_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_resample_num_weights(us_resample_handle h);
const char* us_resample_weight_key(us_resample_handle h, int i);
const char* us_resample_last_error(us_resample_handle h);
/* samples of the output for T input samples: (new_freq * T + orig_freq - 1) / orig_freq in 64-bit integers (0 for T < 1) */
int64_t us_resample_out_length(us_resample_handle h, int64_t T);
size_t us_resample_workspace_bytes(us_resample_handle h, int B, int Tmax);
/* wav [B][Tmax] (device); lengths: HOST int64 [B], the samples of each item in [1, Tmax], or NULL for Tmax each; Tmax at most 2^30.
 * Samples at or past an item's length are never read.  out [B][us_resample_out_length(h, Tmax)]: item b has
 * us_resample_out_length(h, lengths[b]) samples, the ones past them are 0; nothing past the row is written. */
int us_resample_forward(us_resample_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, float* out, void* workspace,
                        size_t workspace_bytes, us_stream stream);

/* ---- HuBERT encoder (the unit extractor's dense model, textless/data/hubert_feature_reader.py, and the ContentVec extractor of
 * scripts/voice_conversion.py:46-68), csrc/hubert.hip ---------------------------------------------------------------------------------
 * 16 kHz waveform [B][Tmax] with per-item lengths -> the encoder's state after n layers, [B][F][H] with F = us_hubert_frames(h, Tmax):
 * transformers.HubertModel with the group-norm feature extractor and post-LN layers (hidden_states[n]; fairseq's output_layer = n), eval
 * mode.  Weights go in by transformers' state_dict keys, except that the positional convolution's weight-norm pair is given folded as
 * "encoder.pos_conv_embed.conv.weight" = g v / |v| [H][H / groups][k] and masked_spec_embed is not taken.  fp32 storage, exact fp32
 * products on the matrix cores.  Same conventions as the other weight-table handles: us_hubert_create touches no device, the caller owns
 * the scratch (us_hubert_workspace_bytes, 0 for B < 1 or a Tmax below the receptive field), us_hubert_forward allocates nothing and only
 * enqueues on `stream` (lengths are read on the host during the call), a call made while another device than the handle's is current is
 * refused (US_EINVAL), and an item alone or in a batch, and repeated calls, give the same bits.
 * us_hubert_create returns US_EINVAL for feat_extract_norm other than US_HUBERT_NORM_GROUP, do_stable_layer_norm, a hidden size the heads
 * do not divide, a head dimension above 64 or not a multiple of 4, a hidden size the positional groups do not divide, more than
 * US_HUBERT_MAX_CONV extractor layers, more than 16 taps in layer 0 or a stride above 4 in a later layer. */
#define US_HUBERT_MAX_CONV 8
enum { US_HUBERT_NORM_GROUP = 0, US_HUBERT_NORM_LAYER = 1 };
typedef struct us_hubert* us_hubert_handle;
typedef struct us_hubert_config {
  int32_t n_conv;                            /* 7 */
  int32_t conv_dim[US_HUBERT_MAX_CONV];      /* 512 x 7 */
  int32_t conv_kernel[US_HUBERT_MAX_CONV];   /* 10, 3, 3, 3, 3, 2, 2 */
  int32_t conv_stride[US_HUBERT_MAX_CONV];   /* 5, 2, 2, 2, 2, 2, 2 */
  int32_t hidden_size;                       /* 768 */
  int32_t n_heads;                           /* 12 */
  int32_t intermediate_size;                 /* 3072 */
  int32_t n_layers;                          /* 12 */
  int32_t pos_conv_kernel;                   /* 128; padding k / 2, an even k drops the last output step */
  int32_t pos_conv_groups;                   /* 16 */
  int32_t feat_extract_norm;                 /* US_HUBERT_NORM_GROUP */
  int32_t do_stable_layer_norm;              /* 0 */
  float layer_norm_eps;                      /* 1e-5 */
} us_hubert_config;
int us_hubert_create(us_hubert_handle* out, const us_hubert_config* cfg);
int us_hubert_destroy(us_hubert_handle h);
int us_hubert_load_weight(us_hubert_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_hubert_num_weights(us_hubert_handle h);
const char* us_hubert_weight_key(us_hubert_handle h, int i);
const char* us_hubert_last_error(us_hubert_handle h);
/* frames of a T-sample item: floor((L - k) / s) + 1 through the extractor's layers (320 samples per frame, 400 for the first, with the
 * base values); US_EINVAL (negative) when T is shorter than the receptive field */
int us_hubert_frames(us_hubert_handle h, int64_t T);
size_t us_hubert_workspace_bytes(us_hubert_handle h, int B, int Tmax);
/* wav [B][Tmax] (device); lengths: HOST int64 [B], the samples of each item, at least the receptive field (else US_EINVAL) and at most
 * Tmax, or NULL for Tmax each.  Item b's rows are what the model gives for its own samples alone: the group norm's statistics run over its
 * own steps, the positional convolution sees zeros past its last frame, attention runs over its own frames (this is not the behaviour of
 * transformers' attention_mask); samples at or past its length are never read.
 * normalize: the reader's F.layer_norm(x, x.shape) first, per item over its own samples.  n_layers_out in [0, n_layers]: stop after that
 * many layers.  out [B][F][H]; hidden_states: NULL, or [B][n_layers_out + 1][F][H] receiving the state after 0 .. n_layers_out layers.  Rows
 * at and past an item's frames are 0; nothing past the tensors is written. */
int us_hubert_forward(us_hubert_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out, float* out,
                      float* hidden_states, void* workspace, size_t workspace_bytes, us_stream stream);

/* ---- WavLM encoder (the upstream of the speaker embedder, ECAPA_TDNN_SMALL(feat_type="wavlm_large")), csrc/hubert.hip ---------------------
 * transformers.WavLMModel in eval mode, in both published forms: feat_extract_norm = US_HUBERT_NORM_LAYER with do_stable_layer_norm = 1 and
 * conv_bias = 1 (WavLM-large: every extractor layer is conv + bias, LayerNorm over channels, GELU; the encoder is pre-LN, so hidden state
 * i < L is the un-normalised input of layer i and hidden state L is encoder.layer_norm of the stream), or US_HUBERT_NORM_GROUP with 0 and 0
 * (WavLM-base and base-plus: HuBERT's schedule).  Any other combination of the three is US_EINVAL, as are the geometries us_hubert_create
 * refuses, an odd num_buckets or one outside [4, 4096], and a max_bucket_distance not above num_buckets / 4.
 * Attention adds WavLM's gated relative position bias: score = q.k d^-1/2 + gate[q] * rel_attn_embed[bucket(k - q)][head], with the gate
 * a (b gru_rel_pos_const[head] - 1) + 2, a and b the sigmoids of the two sums of four of gru_rel_pos_linear(x_head), x the attention's
 * input.  The delta -> bucket map is made on the host at create; from layer 0's rel_attn_embed a per-head table over delta in [-D, D] is
 * formed, D the first saturated distance (778 at the default 320 / 800), and larger distances are clamped: no [F][F] array exists.
 * Weights go in by transformers' state_dict keys (positional convolution folded, masked_spec_embed not taken), as for us_hubert_*, whose
 * conventions and per-item semantics hold here too. */
typedef struct us_wavlm* us_wavlm_handle;
typedef struct us_wavlm_config {
  int32_t n_conv;                            /* 7 */
  int32_t conv_dim[US_HUBERT_MAX_CONV];      /* 512 x 7 */
  int32_t conv_kernel[US_HUBERT_MAX_CONV];   /* 10, 3, 3, 3, 3, 2, 2 */
  int32_t conv_stride[US_HUBERT_MAX_CONV];   /* 5, 2, 2, 2, 2, 2, 2 */
  int32_t hidden_size;                       /* 1024 */
  int32_t n_heads;                           /* 16 */
  int32_t intermediate_size;                 /* 4096 */
  int32_t n_layers;                          /* 24 */
  int32_t pos_conv_kernel;                   /* 128 */
  int32_t pos_conv_groups;                   /* 16 */
  int32_t feat_extract_norm;                 /* US_HUBERT_NORM_LAYER */
  int32_t do_stable_layer_norm;              /* 1 */
  float layer_norm_eps;                      /* 1e-5 */
  int32_t conv_bias;                         /* 1 */
  int32_t num_buckets;                       /* 320 */
  int32_t max_bucket_distance;               /* 800 */
} us_wavlm_config;
int us_wavlm_create(us_wavlm_handle* out, const us_wavlm_config* cfg);
int us_wavlm_destroy(us_wavlm_handle h);
int us_wavlm_load_weight(us_wavlm_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_wavlm_num_weights(us_wavlm_handle h);
const char* us_wavlm_weight_key(us_wavlm_handle h, int i);
const char* us_wavlm_last_error(us_wavlm_handle h);
int us_wavlm_frames(us_wavlm_handle h, int64_t T);
size_t us_wavlm_workspace_bytes(us_wavlm_handle h, int B, int Tmax);
/* the bucket of delta = key - query in the handle's host map (|delta| beyond the first saturated distance is clamped to it) */
int us_wavlm_position_bucket(us_wavlm_handle h, int64_t delta);
/* The arguments and per-item semantics of us_hubert_forward.  hidden_states (or NULL): state l of item b is written at
 * hidden_states + b * hs_item_stride + l * hs_layer_stride (floats), [F][H] each: ((n_layers_out + 1) F H, F H) is [B][n + 1][F][H],
 * transformers' order, and (F H, B F H) is [n + 1][B][F][H], what us_speaker_forward reads.  Strides under which two states would overlap
 * are US_EINVAL. */
int us_wavlm_forward(us_wavlm_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out, float* out,
                     float* hidden_states, int64_t hs_item_stride, int64_t hs_layer_stride, void* workspace, size_t workspace_bytes,
                     us_stream stream);

/* ---- Whisper recogniser (transformers.WhisperForConditionalGeneration, eval mode), csrc/whisper.hip + the encoder schedule in csrc/hubert.hip --
 * log-mel features [B][n_mels][2 S] (S = max_source_positions) -> encoder hidden states, teacher-forced logits, or greedy token ids.  fp32
 * storage and exact-fp32 products on the matrix cores.  The model, as transformers computes it:
 *   encoder stem: GELU(conv1) (k 3, padding 1), GELU(conv2) (k 3, stride 2, padding 1), + embed_positions; the input has exactly 2 S frames;
 *   encoder layers, then layer_norm: x += out_proj(attn(LN(x))) with q scaled by d_head^-1/2 and k_proj without bias, x += fc2(GELU(fc1(LN(x))));
 *     GELU is the erf form, LayerNorm's eps is 1e-5;
 *   decoder input: embed_tokens[id] + embed_positions[pos];
 *   decoder layers: pre-LN causal self-attention, pre-LN cross-attention over the encoder's output, pre-LN MLP;
 *   decoder end: layer_norm, then logits = h . embed_tokens^T.
 * Weights go in by the state_dict keys model.encoder.* and model.decoder.* (us_whisper_weight_key lists them); proj_out.weight is the tied
 * model.decoder.embed_tokens.weight and is not taken.  Same conventions as the other weight-table handles: us_whisper_create touches no
 * device, the caller owns the scratch (us_whisper_workspace_bytes(h, B), 0 for B outside [1, 65535]), the computing calls allocate nothing and
 * enqueue on `stream` (us_whisper_generate also waits for the stream every 8 steps, to read how many items still run), a call made while
 * another device than the handle's is current is refused (US_EINVAL), and an item alone or in a batch, and repeated calls, give the same bits
 * (logits and tokens).
 * us_whisper_create returns US_EINVAL for a d_model the heads do not divide, a head dimension above 64 or not a multiple of 4, a decoder
 * feed-forward size that is no multiple of 4, and max_source_positions or max_target_positions above 2048.
 * us_whisper_generate is plain greedy decoding (callers put <|notimestamps|> in the prompt); us_whisper_decode is greedy decoding under the
 * timestamp rules, what openai's `whisper.decode(model, mel, DecodingOptions())` runs by default (without_timestamps=False).
 * us_whisper_decode_beam is beam search under those rules (DecodingOptions(beam_size=n, patience=p)).
 * Not built: temperature fallback, fp16 weights. */
typedef struct us_whisper* us_whisper_handle;
typedef struct us_whisper_config {
  int32_t n_mels;
  int32_t d_model;
  int32_t encoder_layers, encoder_heads, encoder_ffn;
  int32_t decoder_layers, decoder_heads, decoder_ffn;
  int32_t max_source_positions;      /* S */
  int32_t max_target_positions;
  int32_t vocab_size;
} us_whisper_config;
int us_whisper_create(us_whisper_handle* out, const us_whisper_config* cfg);
int us_whisper_destroy(us_whisper_handle h);
int us_whisper_load_weight(us_whisper_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream);
int us_whisper_num_weights(us_whisper_handle h);
const char* us_whisper_weight_key(us_whisper_handle h, int i);
const char* us_whisper_last_error(us_whisper_handle h);
size_t us_whisper_workspace_bytes(us_whisper_handle h, int B);
/* features [B][n_mels][T] (device), T = 2 S else US_EINVAL -> out [B][S][d_model], the encoder's last hidden state */
int us_whisper_encode(us_whisper_handle h, const float* features, int B, int T, float* out, void* workspace, size_t workspace_bytes,
                      us_stream stream);
/* teacher forcing: ids HOST int64 [B][N], 1 <= N <= max_target_positions, every id in [0, vocab_size) else US_EINVAL -> logits
 * [B][N][vocab_size] (device), row t the distribution of the token after ids[.][0 .. t].  The positions are walked one by one through the
 * kernels of us_whisper_generate, so these are the bits the greedy loop sees. */
int us_whisper_decoder_logits(us_whisper_handle h, const float* features, int B, int T, const int64_t* ids, int N, float* logits,
                              void* workspace, size_t workspace_bytes, us_stream stream);
/* greedy decoding: prompt HOST int64 [B][P] (P >= 1, teacher-forced), at most max_new tokens per item with P + max_new <=
 * max_target_positions, ended by eos.  suppress / begin_suppress: device bytes [vocab_size] or NULL, non-zero = the token is never chosen /
 * not chosen at the first generated position.  -> tokens [B][max_new] int64 (device), eos at and after an item's end, and n [B] int64, the
 * tokens in front of it.  The token is torch.argmax's: the lower index on an exact tie. */
int us_whisper_generate(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P, int max_new, int64_t eos,
                        const unsigned char* suppress, const unsigned char* begin_suppress, int64_t* tokens, int64_t* n, void* workspace,
                        size_t workspace_bytes, us_stream stream);

/* Greedy decoding under the timestamp rules (openai's SuppressTokens, SuppressBlank, ApplyTimestampRules and GreedyDecoder.update at
 * temperature 0; transformers' WhisperTimeStampLogitsProcessor is the same rule text).  With tb = no_timestamps + 1, the first timestamp token,
 * and an item's sampled tokens so far:
 *   no_timestamps is never chosen; last_ts: at least one token sampled and the last one >= tb; pen_ts: fewer than two sampled, or the
 *   penultimate one >= tb.  last_ts && pen_ts: every token >= tb is masked.  last_ts && !pen_ts: every token < eos is masked (tokens in
 *   [eos, tb) stay allowed).  After any timestamp, with `last` the last one sampled: [tb, last) is masked when last_ts && !pen_ts, else
 *   [tb, last + 1).  At the first generated position every token < tb is masked, and with max_initial_timestamp_index >= 0 every token
 *   > tb + index.  Then, if the log-sum-exp of the surviving timestamp logits is strictly greater than the largest surviving text logit,
 *   all text is masked (equality keeps text; an empty side is -inf).  The token is the argmax of what survives, the lower index on an exact
 *   tie; its log-probability is x[token] - logsumexp(surviving logits).  Where nothing survives the item ends with eos at log-probability 0.
 * An item ends at eos; the log-probabilities of all its steps, the one that emits eos included, are summed into sum_logprobs.  The stage is
 * two launches per step (partial sums over chunks of 512 logits, then one workgroup per item), without atomics on floats: an item has the
 * same bits alone, in any batch and in repeated calls. */
typedef struct us_whisper_decode_options {
  int32_t eos;                          /* 0 <= eos < no_timestamps */
  int32_t no_timestamps;                /* no_timestamps + 1 < vocab_size */
  int32_t max_initial_timestamp_index;  /* -1: none */
  int32_t no_speech;                    /* -1: none; else no_speech_prob is computed */
  int32_t sot_index;                    /* the start token's place in the prompt, in [0, P): where no_speech_prob is read */
  int32_t max_new;                      /* us_whisper_decode: P + max_new <= max_target_positions */
} us_whisper_decode_options;
/* As us_whisper_generate (prompt on the host, nothing allocated, the stream awaited every 8 steps), under the rules above.  -> tokens
 * [B][max_new] int64 with eos at and after an item's end, n [B] int64, sum_logprobs [B] fp32 and, when options->no_speech >= 0,
 * no_speech_prob [B] fp32 = softmax(unmasked logits after prompt[.][sot_index])[no_speech] (one more vocabulary GEMM); all on the device.
 * US_EINVAL for eos >= no_timestamps, no_timestamps + 1 >= vocab_size, sot_index outside the prompt, P + max_new beyond
 * max_target_positions.  The workspace is us_whisper_workspace_bytes(h, B), which includes the stage's state and partials. */
int us_whisper_decode(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P,
                      const us_whisper_decode_options* options, const unsigned char* suppress, const unsigned char* begin_suppress,
                      int64_t* tokens, int64_t* n, float* sum_logprobs, float* no_speech_prob, void* workspace, size_t workspace_bytes,
                      us_stream stream);
/* One selection step without a handle, through the same two kernels: logits [B][V] (device, any B >= 1, walked in groups of 16), the
 * histories HOST [B], masks as above -> token [B] int64, logprob [B] fp32, decided_timestamp [B] int32 (1: the timestamps won the decision),
 * on the device.  A done item returns eos, 0 and 0.  options->eos, no_timestamps and max_initial_timestamp_index are read.  scratch: device,
 * us_whisper_select_scratch_bytes(V). */
typedef struct us_whisper_history {
  int32_t n_sampled;                    /* tokens sampled so far; 0: the first generated position */
  int32_t last, penultimate;            /* read when n_sampled >= 1 / >= 2 */
  int32_t last_timestamp;               /* the last sampled token >= tb, or -1 */
  int32_t done;
} us_whisper_history;
size_t us_whisper_select_scratch_bytes(int V);
int us_whisper_select(const float* logits, int B, int V, const us_whisper_history* history, const us_whisper_decode_options* options,
                      const unsigned char* suppress, const unsigned char* begin_suppress, int64_t* token, float* logprob,
                      int32_t* decided_timestamp, void* scratch, size_t scratch_bytes, us_stream stream);

/* Beam search under the same rules: openai-whisper's BeamSearchDecoder.update / finalize and MaximumLikelihoodRanker with length_penalty=None,
 * what `whisper.decode(model, mel, DecodingOptions(beam_size=n, patience=p))` runs, with max_candidates C = round(n * patience).
 * An item has n rows, each with a sampled sequence, a score (the sum of its log-probabilities, a double) and a live flag; row 0 alone is live at
 * the start.  A pool holds finished (sequence, score) pairs.  At every step each live row offers its top n + 1 surviving tokens by
 * log-probability under the rules above applied to its own sequence (the lower id first on equal values, a token at -inf never, (eos, 0) when
 * nothing survives); the candidates, listed in (row, rank) order, are sorted descending by score + log-probability, equal totals keeping that
 * order, and walked: an eos candidate finishes (the row's sequence without the eos, the total), any other becomes the next new row (parent,
 * token, total), and the walk stops once n new rows exist; what lies behind the stop is ignored, rows not filled are dead.  The finished
 * entries join the pool in walk order while it holds fewer than C.  An item ends when its pool holds C entries, when no row is live, or after
 * max_new steps, whatever the other items of the batch do.  Then a pool of fewer than n entries takes the live rows in descending score (the
 * lower row first), and the entry with the largest score / length wins (length 0 counts as -infinity; the earlier entry on a tie).
 * n = 1 with C = 1 is us_whisper_decode.
 * Rows are item-major; a launch group holds floor(16 / n) whole items, so a step streams the weights once for all their rows.  The cross keys
 * and values are stored once per item; the self cache is stored once per row and never moved: a per-row table names, for every position, the
 * row of the item that holds its key.  An item has the same bits alone, in any batch and in repeated calls.
 * -> tokens [B][max_new] int64 (the winner's sequence, eos at and after its end), n [B] int64 its length, sum_logprobs [B] fp32 its score
 * (the eos term included where it ended by eos), no_speech_prob [B] as us_whisper_decode (the item's first row).  US_EINVAL for beam_size outside
 * [1, 16], max_candidates outside [1, 64], a workspace below us_whisper_beam_workspace_bytes(h, B, beam_size) (0 for arguments out of range),
 * and everything us_whisper_decode refuses. */
size_t us_whisper_beam_workspace_bytes(us_whisper_handle h, int B, int beam_size);
int us_whisper_decode_beam(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P,
                           const us_whisper_decode_options* options, int beam_size, int max_candidates, const unsigned char* suppress,
                           const unsigned char* begin_suppress, int64_t* tokens, int64_t* n, float* sum_logprobs, float* no_speech_prob,
                           void* workspace, size_t workspace_bytes, us_stream stream);
/* One step of the beam stage without a handle, through the same kernels: logits [B * beam_size][V] (device, rows item-major), the rows'
 * histories and scores HOST [B * beam_size] (history.done != 0: the row is dead) -> per item, on the device: the new rows parent / token /
 * score [B][beam_size] (parent -1, token eos, score 0 for a dead row), n_live [B], and the newly finished entries in walk order fin_parent /
 * fin_score [B][beam_size] (-1 / 0 behind n_fin [B]).  scratch: device, us_whisper_beam_select_scratch_bytes(V, beam_size). */
size_t us_whisper_beam_select_scratch_bytes(int V, int beam_size);
int us_whisper_beam_select(const float* logits, int B, int V, int beam_size, const us_whisper_history* history, const double* scores,
                           const us_whisper_decode_options* options, const unsigned char* suppress, const unsigned char* begin_suppress,
                           int32_t* parent, int64_t* token, double* score, int32_t* n_live, int32_t* fin_parent, double* fin_score, int32_t* n_fin,
                           void* scratch, size_t scratch_bytes, us_stream stream);

/* ---- unit extraction from the dense upstream features on, csrc/units.hip ------------------------------------------------------------
 * The reference's host path (finetune.py:112-128: scikit-learn `KMeans.predict`, `torch.unique_consecutive`, util.py:69-102
 * `process_unit`) as handle-free device calls.  Every call only enqueues on `stream`, allocates nothing and takes device scratch of
 * us_units_workspace_bytes(B, Tmax, K, D, Lout) (K = 0: no quantize, Lout = 0: no process).  All integer outputs are exact.
 * us_units_pack_centers: centres [K][D] fp32 (finite) -> `packed` (us_units_packed_bytes): the GEMM operand, 1/2 |c_k|^2 computed in fp64
 *   and rounded once to fp32, and max |c_k|.  K in [1, 2048]; D a multiple of 4 in [4, 1024].
 * us_units_quantize: dense [B][Tmax][D], lengths [B] (device int64) -> units [B][Tmax] int64 = the fp64 argmin over k of
 *   sum_d (x_d - c_kd)^2 taken over the fp32 inputs, the lower index on exact ties.  Scores come from one fp32 matrix-core GEMM whose
 *   epilogue keeps (best, second best, index) per row; a row whose gap is at most twice the proven fp32 error bound is re-evaluated over
 *   all K in fp64 on the device.  Rows t >= lengths[b] get -1; a row with a non-finite feature gets -1.  counters [2] (device int32,
 *   overwritten): [0] rows with a non-finite feature, [1] rows decided in fp64.
 * us_units_dedup: run-length encoding per item, `unique_consecutive(return_counts=True)`: units [B][Tmax] with lengths [B] ->
 *   out_units, out_durations [B][Tmax] (zero beyond n[b]) and n [B], all int64 on the device.  out_units must not alias units.
 * us_units_process: `process_unit(encoded, sampling_rate, hop_length)` in closed form for runs units / durations [B][Lin] (durations NULL:
 *   all ones) with n_in [B] valid entries.  With spf = sampling_rate / 50 (integer division, as the reference), run i holds the samples of
 *   its 50 Hz frames, output frame j covers samples [j hop, (j + 1) hop), there are (sum(durations) spf) / hop of them, and a frame's unit
 *   is the one with the most samples in it (ties: the smallest unit value, `torch.mode`); the frames are then run-length encoded into
 *   out_units, out_durations [B][Lout] int64 (zero beyond n_out[b]), duration_f [B][Lout] fp32 (optional: the `duration` us_tts_align and
 *   generate_path take) and n_out [B] (0 for an input shorter than one hop; -1, and nothing else, for an item with more than Lout output
 *   frames).  An output frame may span up to 64 frames of the 50 Hz stream: US_EINVAL beyond that.
 * us_units_encode: us_units_quantize then us_units_process (durations all ones, n_in = lengths) in one call. */
size_t us_units_packed_bytes(int K, int D);
int us_units_pack_centers(const float* centers, int K, int D, void* packed, size_t packed_bytes, us_stream stream);
size_t us_units_workspace_bytes(int B, int Tmax, int K, int D, int Lout);
int us_units_quantize(const float* dense, const int64_t* lengths, const void* packed, int B, int Tmax, int K, int D, int64_t* units,
                      int32_t* counters, void* workspace, size_t workspace_bytes, us_stream stream);
int us_units_dedup(const int64_t* units, const int64_t* lengths, int B, int Tmax, int64_t* out_units, int64_t* out_durations, int64_t* n,
                   void* workspace, size_t workspace_bytes, us_stream stream);
int us_units_process(const int64_t* units, const int64_t* durations, const int64_t* n_in, int B, int Lin, int sampling_rate, int hop_length,
                     int64_t* out_units, int64_t* out_durations, float* duration_f, int64_t* n_out, int Lout, void* workspace,
                     size_t workspace_bytes, us_stream stream);
int us_units_encode(const float* dense, const int64_t* lengths, const void* packed, int B, int Tmax, int K, int D, int sampling_rate,
                    int hop_length, int64_t* out_units, int64_t* out_durations, float* duration_f, int64_t* n_out, int Lout,
                    int32_t* counters, void* workspace, size_t workspace_bytes, us_stream stream);

/* ---- fitting the unit codebook, csrc/units_fit.hip -----------------------------------------------------------------------------------
 * The half of a k-means iteration that us_units_quantize does not do, as handle-free device calls that only enqueue on `stream` and
 * allocate nothing.  K in [1, 2048], D a multiple of 4 in [4, 1024], at most 2^24 rows per call; the two size functions return 0 for
 * anything else and the calls return US_EINVAL.  No float atomics anywhere: every output has the same bits on every run.
 * us_units_fit_workspace_bytes(rows, K, D): device scratch of one us_units_fit_accumulate or us_units_fit_seed_step call.
 * us_units_fit_state_bytes(K, D): the state that accumulate calls add into: fp64 sums [K][D], int64 counts [K], the fp64 inertia, rows used
 *   and rows skipped.  us_units_fit_state_clear zeroes it; us_units_fit_update leaves it cleared.
 * us_units_fit_accumulate: labels [rows] (device int64, as us_units_quantize writes them: -1 or anything outside [0, K) is a skipped row),
 *   dense [rows][D] fp32 and the centres [K][D] the labels were taken against -> state += {sum of the rows of every centre, their number,
 *   sum_rows sum_d (x_d - c_label,d)^2, rows used, rows skipped}.  An inverted index (per-chunk histograms, an exclusive scan, a stable
 *   scatter of row numbers) gives every centre its rows in ascending order; each row is read once and added in fp64 in that order, lists
 *   longer than 512 rows in pieces of 512 whose partial sums are added in piece order.  The sums depend on how the rows were split into
 *   calls (in the last fp64 bits) and on nothing else.
 * us_units_fit_update: mode US_UNITS_FIT_LLOYD: c_k = fp32(sum_k / count_k), totals_out[k] = count_k (totals may be NULL);
 *   US_UNITS_FIT_MINIBATCH: c_k = fp32((c_k total_k + sum_k) / (total_k + count_k)), totals_out[k] = totals_in[k] + count_k (scikit-learn's
 *   MiniBatchKMeans.partial_fit with reassignment_ratio = 0).  A centre with count_k = 0 keeps its value.  centers_out may be centers_in and
 *   totals_out may be totals_in.  record (device, 40 bytes): {fp64 inertia, fp64 shift2 = sum (c_new - c_old)^2 over the fp32 values,
 *   int64 empty centres, int64 rows used, int64 rows skipped}.
 * us_units_fit_seed_step: step `step` in [0, K) of plain D^2 k-means++ over dense [B][Tmax][D] with lengths [B] (device int64); a row at or
 *   beyond lengths[b] or with a non-finite feature is never chosen.  Step 0 initialises mind [B Tmax] (device fp64, the caller's) and takes
 *   valid row floor(u n_valid); step j >= 1 sets mind_i = min(mind_i, sum_d (x_id - c_d)^2) for centre j - 1 (fp64, d ascending), takes a
 *   fixed-order blocked inclusive scan P and picks the smallest valid i with P_i > u P_last, or valid row floor(u n_valid) when P_last = 0.
 *   u in [0, 1) comes from the caller.  centers [K][D] row `step` and picked[step] (device int64: the row index, -1 without a valid row)
 *   are written; steps must be called in order with the same buffers. */
enum { US_UNITS_FIT_LLOYD = 0, US_UNITS_FIT_MINIBATCH = 1 };
size_t us_units_fit_workspace_bytes(int64_t rows, int K, int D);
size_t us_units_fit_state_bytes(int K, int D);
int us_units_fit_state_clear(void* state, size_t state_bytes, int K, int D, us_stream stream);
int us_units_fit_accumulate(const float* dense, const int64_t* labels, const float* centers, int64_t rows, int K, int D, void* state,
                            size_t state_bytes, void* workspace, size_t workspace_bytes, us_stream stream);
int us_units_fit_update(int mode, const float* centers_in, float* centers_out, const int64_t* totals_in, int64_t* totals_out, int K, int D,
                        void* state, size_t state_bytes, void* record, us_stream stream);
int us_units_fit_seed_step(const float* dense, const int64_t* lengths, int B, int Tmax, int K, int D, int step, double u, double* mind,
                           float* centers, int64_t* picked, void* workspace, size_t workspace_bytes, us_stream stream);

/* ---- the recogniser's end: CTC head, greedy decoding, edit distance, csrc/ctc.hip ------------------------------------------------------
 * What scoring synthesised speech by CER / WER needs after the encoder (us_hubert_forward), as handle-free device calls that only
 * enqueue on `stream`, allocate nothing and need no scratch.  V in [2, 2048], H a multiple of 4 in [4, 1024], B <= 65535 and at most 2^24
 * rows per call; us_ctc_packed_bytes returns 0 for anything else and the calls return US_EINVAL.
 * us_ctc_pack_head: `lm_head` weight [V][H] and bias [V] (NULL: zeros) -> `packed` (us_ctc_packed_bytes): the GEMM operand and the bias.
 * us_ctc_logits: hidden [B][Tmax][H], lengths [B] (device int64, frames per item; NULL: all Tmax) -> logits [B][Tmax][V] =
 *   hidden . weight^T + bias in fp32 on the matrix cores, a row's products added in a fixed order that does not depend on where the row
 *   lies (an item has the same bits alone and in a batch); log_probs [B][Tmax][V] (optional) = log_softmax over V; ids [B][Tmax] int64
 *   (optional) = the argmax of the logits as written, the lower index on ties (finite logits).  Rows t >= lengths[b] get logits 0,
 *   log_probs 0 and ids -1, and their features are not read.
 * us_ctc_collapse: greedy CTC decoding per item over ids [B][Tmax] with lengths [B] (NULL: all Tmax): equal neighbours are merged,
 *   then `blank` is dropped -> tokens [B][Tmax] and first_frame [B][Tmax] (optional: the frame at which each kept token's run starts),
 *   zero beyond n[b], and n [B], all int64 on the device.  tokens and first_frame must not alias ids.
 * us_edit_distance: Levenshtein distance (unit costs) of P pairs hyp [P][Lh] / ref [P][Lr] with n_hyp, n_ref [P] valid tokens (clamped to
 *   [0, Lh] and [0, Lr]) -> dist [P], exact, all int64 on the device.  Lh and Lr at most 4096, else US_EINVAL; P = 0 does nothing.  Only
 *   the distance: substitution / deletion / insertion counts depend on which optimal alignment is taken. */
size_t us_ctc_packed_bytes(int V, int H);
int us_ctc_pack_head(const float* weight, const float* bias, int V, int H, void* packed, size_t packed_bytes, us_stream stream);
int us_ctc_logits(const float* hidden, const int64_t* lengths, const void* packed, int B, int Tmax, int V, int H, float* logits,
                  float* log_probs, int64_t* ids, us_stream stream);
int us_ctc_collapse(const int64_t* ids, const int64_t* lengths, int B, int Tmax, int64_t blank, int64_t* tokens, int64_t* first_frame,
                    int64_t* n, us_stream stream);
int us_edit_distance(const int64_t* hyp, const int64_t* n_hyp, int Lh, const int64_t* ref, const int64_t* n_ref, int Lr, int P, int64_t* dist,
                     us_stream stream);

/* ---- fitting the CTC head: loss, gradient, the head's backward pass, forced alignment, csrc/ctc_train.hip -----------------------------
 * Handle-free device calls like the ones above: they allocate nothing and only enqueue on `stream`.  Scratch is the caller's, at least
 * what the matching *_workspace_bytes host function returns (0 for sizes the call refuses); it may hold anything and is reusable as soon
 * as the call's work on the stream is done.  B <= 65535, at most 2^24 rows (B * Tmax) per call, V in [2, 2048], blank in [0, V).  A target
 * holds at most 1024 tokens: Lmax > 1024 is US_EINVAL.  frame_lengths [B] (NULL: all Tmax), targets [B][Lmax] and target_lengths [B] are
 * device int64; lengths are clamped to [0, Tmax] and [0, Lmax].  The extended label sequence of an item with L tokens has S = 2 L + 1
 * states (blank, token 0, blank, ..., blank).
 * us_ctc_loss: logits [B][Tmax][V] fp32 (the log-softmax over V is taken inside) -> loss [B] = -log p(target | logits), and, when
 *   grad_logits [B][Tmax][V] is not NULL, d(sum_b grad_out[b] loss[b]) / d logits = grad_out[b] * (softmax - occupancy); grad_out [B] device
 *   fp32, NULL: ones.  with_grad of the workspace size says whether grad_logits will be given.  stage = US_CTC_WHOLE is the complete call.
 *   A training step that learns grad_out only after the loss splits it: US_CTC_FORWARD (grad_logits NULL, workspace sized with_grad = 1)
 *   writes the loss and leaves alpha in the workspace; US_CTC_BACKWARD (grad_logits given), with the same arguments and that untouched
 *   workspace, runs the backward sweep alone and may be repeated.  The two give the bits of the whole call.  Rows t >= frame_lengths[b]
 *   get gradient 0 and are not read.  An item has the same loss and gradient bits alone and inside any batch, and from run to run: the occupancy of a
 *   vocabulary entry that occurs several times in the target is added in ascending target position, the blank's in a fixed tree over the
 *   states; there are no float atomics.  An infeasible item (fewer frames than L + the number of adjacent equal target pairs) gets loss
 *   +inf (0 when zero_infinity != 0) and gradient 0 -- torch.nn.functional.ctc_loss writes NaN gradients there unless zero_infinity is set.
 *   L = 0 is valid (the all-blank path); so is T = 0 with L = 0 (loss 0).  A target outside [0, V) or equal to the blank makes its item's
 *   loss NaN and its gradient 0; nothing is read out of bounds.
 * us_ctc_head_backward: grad_logits [B][Tmax][V], hidden [B][Tmax][H] (H a multiple of 4 in [4, 1024]), lengths as in us_ctc_logits ->
 *   d_weight [V][H] = sum over live rows of g[row][v] hidden[row][h], d_bias [V] = sum of g[row][v], and, when d_hidden is not NULL,
 *   d_hidden [B][Tmax][H] = g . weight (weight [V][H] as given to us_ctc_pack_head; needed only then).  Both products run on the fp32 matrix
 *   cores.  Rows t >= lengths[b] are not read, contribute nothing and get d_hidden 0.  The sum over rows is taken per chunk of rows into
 *   the workspace and the chunks are then added in order: the same bits in every run (the chunking depends on B * Tmax).
 * us_ctc_forced_align: scores [B][Tmax][V] fp32 (log-probabilities, or any additive score) -> the best path through the states: path
 *   [B][Tmax] int64 = the vocabulary entry emitted at each frame, blank included, -1 at t >= frame_lengths[b]; score [B] = the sum of the
 *   path's scores, added in frame order in fp32; start [B][Lmax] and frames [B][Lmax] int64 = the first frame of each target token and the
 *   number of frames on it (0 beyond target_lengths[b]).  Tie rule: among equal predecessors staying in s wins over s - 1, and s - 1 over
 *   s - 2; of the two end states the last label wins over the final blank.  An infeasible item gets score -inf, a path of -1 and frames 0;
 *   a target outside [0, V) or equal to the blank gives score NaN and the same. */
enum { US_CTC_WHOLE = 0, US_CTC_FORWARD = 1, US_CTC_BACKWARD = 2 };
size_t us_ctc_loss_workspace_bytes(int B, int Tmax, int Lmax, int with_grad);
int us_ctc_loss(const float* logits, const int64_t* frame_lengths, const int64_t* targets, const int64_t* target_lengths, const float* grad_out,
                int B, int Tmax, int V, int Lmax, int64_t blank, int zero_infinity, int stage, float* loss, float* grad_logits, void* workspace,
                size_t workspace_bytes, us_stream stream);
size_t us_ctc_head_backward_workspace_bytes(int B, int Tmax, int V, int H);
int us_ctc_head_backward(const float* grad_logits, const float* hidden, const int64_t* lengths, const float* weight, int B, int Tmax, int V,
                         int H, float* d_weight, float* d_bias, float* d_hidden, void* workspace, size_t workspace_bytes, us_stream stream);
size_t us_ctc_align_workspace_bytes(int B, int Tmax, int Lmax);
int us_ctc_forced_align(const float* scores, const int64_t* frame_lengths, const int64_t* targets, const int64_t* target_lengths, int B, int Tmax,
                        int V, int Lmax, int64_t blank, int64_t* path, float* score, int64_t* start, int64_t* frames, void* workspace,
                        size_t workspace_bytes, us_stream stream);

/* ---- active speech level and gain normalisation: ITU-T P.56 method B, what `sv56` does, csrc/level.hip ---------------------------------
 * Handle-free device calls like the ones above: they allocate nothing, only enqueue on `stream`, and nothing is read back between
 * measuring and applying.  Scratch is the caller's, at least us_level_workspace_bytes(B, Tmax) (0 for what the calls refuse); it may hold
 * anything, and the two calls may share it.  B in [1, 65535], Tmax in [1, 2^30], sample_rate > 0, dtypes US_LEVEL_F32 (samples in units of
 * full scale) or US_LEVEL_I16 (s / 32768); anything else is US_EINVAL.  wav [B][Tmax]; lengths [B] device int64, clamped to [0, Tmax],
 * NULL: every item has Tmax samples; samples at or past an item's length are never read.  quantize_input != 0 (fp32 input only) first
 * takes the reference's route to int16, trunc(x * 32767) with the product in fp32, held to the int16 range.
 * The measurement, all in fp64: g = exp(-1 / (0.03 f)); p[k] = g p[k-1] + (1-g) |x[k]|, q[k] = g q[k-1] + (1-g) p[k] from p = q = 0;
 * thresholds c[j] = 2^(j-15), j = 0..14; a[j] = the number of k with k - last_j(k) <= I = floor(0.2 f + 0.5), last_j(k) the last index <= k
 * with q >= c[j] (nothing is counted before the first); A[j] = 10 log10(sum x^2 / a[j] + 1e-20) (a[j] = 0 taken as 1e-20), D[j] = A[j] -
 * 20 log10 c[j]; the level is A interpolated linearly at D = 15.9 dB on the first segment [j-1, j] with D[j] <= 15.9; -100 when a[0] = 0,
 * D[0] < 15.9 or there is no such segment.  An item is cut into chunks of us_level_chunk() samples from its own start and the chunks are
 * combined in order by separate launches (no workgroup waits for another): an item has the same bits alone, inside any batch and from
 * run to run.
 * us_level_measure: -> stats [B][8] fp64 = level_db, activity = 10^((rms_db - level_db) / 10) (0 at level -100), rms_db = 10 log10(sum x^2
 *   / n + 1e-20), peak = max |x|, mean, max, min, n; counts [B][15] int64 = a (optional).  An item of length 0: level -100, activity 0,
 *   rms_db -100, the rest 0.  An item with a non-finite sample: level, activity, rms_db and peak NaN, counts 0.
 * us_level_apply: wav, in_dtype, quantize_input and lengths as given to us_level_measure, stats as it wrote them -> out [B][Tmax] of
 *   out_dtype: factor = 10^((ndb - level_db) / 20), or 1 when the level is -100 or NaN (such an item comes back unchanged).  fp32 out =
 *   x * factor computed in fp64 and rounded once, not clamped; int16 out = x * factor * 32768 rounded half away from zero and saturated
 *   to [-32768, 32767], a saturated sample counting as clipped.  Samples at or past an item's length are written as 0, nothing past the
 *   row.  gain [B] fp64 = factor and clipped [B] int64 (both optional).  16-byte loads and stores when wav and out are 16-byte aligned and
 *   Tmax is a multiple of 8, single samples otherwise, with the same values.  out must not overlap wav. */
enum { US_LEVEL_F32 = 0, US_LEVEL_I16 = 1 };
int us_level_chunk(void);
size_t us_level_workspace_bytes(int B, int Tmax);
int us_level_measure(const void* wav, int in_dtype, int quantize_input, const int64_t* lengths, int B, int Tmax, int sample_rate, double* stats,
                     int64_t* counts, void* workspace, size_t workspace_bytes, us_stream stream);
int us_level_apply(const void* wav, int in_dtype, int quantize_input, const int64_t* lengths, int B, int Tmax, const double* stats, double ndb,
                   void* out, int out_dtype, double* gain, int64_t* clipped, void* workspace, size_t workspace_bytes, us_stream stream);

/* ---- MOS predictor: the layer mix and the downstream head of s3prl's `mos_wav2vec2`, csrc/mos.hip -----------------------------------------
 * Handle-free device calls like the ones above: they allocate nothing and only enqueue on `stream`.  n_states in [1, 32] hidden states of
 * width H, a multiple of 4 in [4, 1024]; a connector of P in [1, 4096] rows; anything else: us_mos_packed_bytes returns 0 and the calls
 * US_EINVAL.  With s = softmax(weights) over the states and hh[t] = sum_l s_l h_l[t]: z[t] = C hh[t] + c, e[t] = a . z[t] + a0, alpha =
 * softmax_t(e) over the item's own frames, mu[t] = m . z[t] + m0, score = sum_t alpha_t mu[t]; without attention pooling alpha_t = 1 / F and
 * the score is the mean of mu.  With `clipping` the score becomes 2 tanh(score) + 3.
 * us_mos_pack_head: weights [n_states], connector_weight [P][H] and connector_bias [P] (C, c), attention_weight [P] and attention_bias [1]
 *   (a, a0; attention_weight NULL: no attention pooling, attention_bias must then be NULL too), mean_weight [P] and mean_bias [1] (m, m0),
 *   all on the device, a NULL bias standing for zeros -> `packed` (us_mos_packed_bytes, 16-byte aligned): s, v_e = C^T a, v_m = C^T m,
 *   k_e = a . c + a0, k_m = m . c + m0 and the variant.  The softmax and every sum over p (ascending) run in fp64 and are rounded to fp32 once.
 *   us_mos_unpack_head writes them back out (s [n_states], v_e [H], v_m [H], k [2] = k_e, k_m; each optional): NaN when n_states or H are
 *   not the pack's.
 * us_mos_score: hidden state l of item b is [Tmax][H] rows (H contiguous) at hidden + b * item_stride + l * state_stride (elements; both
 *   strides non-negative multiples of 4, hidden 16-byte aligned): `us_hubert_forward`'s [B][L+1][F][H] and `us_wavlm_forward`'s
 *   [L+1][B][F][H] are read in place.  lengths [B] device int64 (frames per item, clamped to [0, Tmax]; NULL: all Tmax); n_states and H as
 *   packed (another head's pack gives NaN scores and is not read past its header) -> scores [B]; optionally frame_scores [B][Tmax] = mu and
 *   attention [B][Tmax] = alpha (1 / F without attention pooling).  Rows at or past an item's length are never read; their frame_scores and
 *   attention entries are written as 0; nothing is written past a row.  AN ITEM OF 0 FRAMES GETS A QUIET NaN, as the mean of nothing is in
 *   torch.  The softmax is taken over e - k_e (it does not change when a constant is added to every e), so a large a0 costs no bits.
 *   workspace: at least us_mos_workspace_bytes(B, Tmax) (0 for what the call refuses: B in [1, 65535], B * Tmax <= 2^24), 8-byte aligned.
 *   No float atomics; every order of summation is a function of H, n_states and the item's own frames alone: an item has the same bits
 *   alone, inside any batch, at any Tmax and from run to run. */
size_t us_mos_packed_bytes(int n_states, int H, int P);
int us_mos_pack_head(const float* weights, const float* connector_weight, const float* connector_bias, const float* attention_weight,
                     const float* attention_bias, const float* mean_weight, const float* mean_bias, int n_states, int H, int P, void* packed,
                     size_t packed_bytes, us_stream stream);
int us_mos_unpack_head(const void* packed, int n_states, int H, float* s, float* v_e, float* v_m, float* k, us_stream stream);
size_t us_mos_workspace_bytes(int B, int Tmax);
int us_mos_score(const float* hidden, int64_t item_stride, int64_t state_stride, const int64_t* lengths, const void* packed, int B, int Tmax,
                 int n_states, int H, int clipping, float* scores, float* frame_scores, float* attention, void* workspace, size_t workspace_bytes,
                 us_stream stream);

/* Last error message of this handle (or of the library when h == NULL). */
const char* us_last_error(us_handle h);

#ifdef __cplusplus
}
#endif
#endif /* UNITSPEECH_HIP_H */
